"""Record lists for the Bristol writers' tests (rv_bristol_write, rv_bristol_write_device, rv_bristol_writer_*): shared by the host
tests and the GPU tests, so that both sides are asked the same things.  `reverie_amd.bristol.dumps` is the model: `want(case)` is its
answer -- the text, or None where it raises ValueError.  TEST INFRASTRUCTURE."""
from __future__ import annotations

import numpy as np

from reverie_amd.ops import OP_DTYPE

WIRE_OOB, BAD_OP, UNSUPPORTED, ARG = 3, 5, 8, 9
INPUT, RANDOM, ADD, ADDCONST, SUB, SUBCONST, MUL, MULCONST, ASSERTZERO, CONST = range(10)
U32 = 0xFFFFFFFF


def op(opcode, dst=0, a=0, b=0, imm=0, domain=0, reserved=0):
    return (domain, opcode, reserved, dst, a, b, imm)


def prog(ops) -> np.ndarray:
    return np.array(list(ops), dtype=OP_DTYPE) if len(ops) else np.zeros(0, OP_DTYPE)


def inputs(n):
    return [op(INPUT, i) for i in range(n)]


# the five line kinds
XOR = lambda d, a, b: op(ADD, d, a, b)  # noqa: E731
AND = lambda d, a, b: op(MUL, d, a, b)  # noqa: E731
INV = lambda d, a: op(ADDCONST, d, a, 0, 1)  # noqa: E731
EQW = lambda d, a: op(ADDCONST, d, a, 0, 0)  # noqa: E731
EQ = lambda d, bit: op(CONST, d, 0, 0, bit)  # noqa: E731
SHORTEST = EQ(0, 0)  # "1 1 0 0 EQ\n": 11 bytes
LONGEST = XOR(U32, U32 - 1, U32 - 2)  # 41 bytes


def random_program(n_in, n_gates, seed, junk=False):
    """a Bristol-shaped program in SSA form; junk: the fields a line does not name hold anything (the writers ignore them)"""
    rng = np.random.default_rng(seed)
    out = inputs(n_in)
    w = n_in
    for _ in range(n_gates):
        k = int(rng.integers(0, 5))
        a, b = (int(rng.integers(0, w)), int(rng.integers(0, w))) if w else (0, 0)
        j = (lambda: int(rng.integers(0, 1 << 32))) if junk else (lambda: 0)
        if k == 0 or not w:
            out.append(op(CONST, w, j(), j(), int(rng.integers(0, 2))))
        elif k == 1:
            out.append(op(ADD, w, a, b, j()))
        elif k == 2:
            out.append(op(MUL, w, a, b, j()))
        else:
            out.append(op(ADDCONST, w, a, j(), k - 3))
        w += 1
    return prog(out)


def digit_boundary_program():
    """every number column crosses every digit-count boundary: 9/10, 99/100, ..., 999 999 999/1 000 000 000, and 2^32 - 1 -- in dst,
    in a and in b (indices are only numbers to a writer: no memory follows them)"""
    vals = [0]
    for k in range(1, 10):
        vals += [10 ** k - 1, 10 ** k]
    vals.append(U32)
    out = inputs(2)
    for v in vals:
        out += [XOR(v, 1, 0), XOR(1, v, 0), XOR(1, 0, v), AND(v, v, v), INV(v, 0), INV(0, v), EQW(v, v), EQ(v, 0), EQ(v, 1)]
    return prog(out)


def ok_cases():
    """[(name, program, n_outputs, n_wires or None)]: lists `dumps` writes"""
    cases = [
        ("empty", prog([]), 0, None),
        ("inputs-only", prog(inputs(7)), 3, None),
        ("no-inputs", prog([EQ(0, 1), INV(1, 0)]), 1, None),
        ("xor", prog(inputs(2) + [XOR(2, 0, 1)]), 1, None),
        ("and", prog(inputs(2) + [AND(2, 1, 0)]), 1, None),
        ("inv", prog(inputs(1) + [INV(1, 0)]), 1, None),
        ("eqw", prog(inputs(1) + [EQW(1, 0)]), 1, None),
        ("eq", prog(inputs(1) + [EQ(1, 1)]), 0, None),
        ("shortest-longest", prog([SHORTEST, LONGEST, SHORTEST, SHORTEST, LONGEST, LONGEST]), 0, None),
        ("digits", digit_boundary_program(), 2, None),
        ("random-a", random_program(5, 35, 1), 4, None),
        ("random-junk", random_program(3, 60, 2, junk=True), 0, None),
        ("random-no-inputs", random_program(0, 20, 3), 0, None),
        ("stated-wires", random_program(4, 12, 4), 2, 16),  # (dumps derives: the case goes through want_stated)
        ("wide-inputs", prog(inputs(300) + [XOR(300, 299, 0)]), 300, None),
    ]
    return cases


def bad_cases():
    """[(name, program, n_outputs, n_wires or None, code)]: one case per defect of the error rule, pairs of defects (the first in
    list order wins; inside one record BAD_OP before UNSUPPORTED before WIRE_OOB), a stated n_wires one too small, one output too
    many.  `dumps` raises ValueError for every one of them (a stated n_wires: dumps derives more wires than stated)."""
    base = inputs(3) + [XOR(3, 0, 1), AND(4, 3, 2)]
    cases = [
        ("reserved", base + [op(ADD, 5, 0, 1, 0, 0, 1)], 0, None, BAD_OP),
        ("reserved-input", [op(INPUT, 0, reserved=7)] + inputs(3)[1:], 0, None, BAD_OP),
        ("domain-4", base + [op(ADD, 5, 0, 1, domain=4)], 0, None, BAD_OP),
        ("domain-255", base + [op(ADD, 5, 0, 1, domain=255)], 0, None, BAD_OP),
        ("opcode-10", base + [op(10, 5, 0, 1)], 0, None, BAD_OP),
        ("z64-opcode-10", base + [op(10, 5, 0, 1, domain=1)], 0, None, BAD_OP),
        ("z64", base + [op(ADD, 5, 0, 1, domain=1)], 0, None, UNSUPPORTED),
        ("z64-input-first", [op(INPUT, 0, domain=1)], 0, None, UNSUPPORTED),
        ("b2a", base + [op(0, 0, 0, domain=2)], 0, None, UNSUPPORTED),
        ("b2a-opcode-99", base + [op(99, 0, 0, domain=2)], 0, None, UNSUPPORTED),  # (the opcode of such a record is not looked at)
        ("sizehint", base + [op(0, 0, 1, 9, domain=3)], 0, None, UNSUPPORTED),
        ("input-behind-run", base + [op(INPUT, 5)], 0, None, UNSUPPORTED),
        ("input-behind-run-then-inputs", base + [op(INPUT, 5), op(INPUT, 6), op(INPUT, 7)], 0, None, UNSUPPORTED),
        ("input-out-of-place", [op(INPUT, 0), op(INPUT, 2), op(INPUT, 1)], 0, None, UNSUPPORTED),
        ("input-first-not-0", [op(INPUT, 1)], 0, None, UNSUPPORTED),
        ("random", base + [op(RANDOM, 5)], 0, None, UNSUPPORTED),
        ("sub", base + [op(SUB, 5, 0, 1)], 0, None, UNSUPPORTED),
        ("subconst", base + [op(SUBCONST, 5, 0, 0, 1)], 0, None, UNSUPPORTED),
        ("mulconst", base + [op(MULCONST, 5, 0, 0, 1)], 0, None, UNSUPPORTED),
        ("assertzero", base + [op(ASSERTZERO, 0, 4)], 0, None, UNSUPPORTED),
        ("addconst-2", base + [op(ADDCONST, 5, 0, 0, 2)], 0, None, UNSUPPORTED),
        ("const-2", base + [op(CONST, 5, 0, 0, 2)], 0, None, UNSUPPORTED),
        ("const-2^63", base + [op(CONST, 5, 0, 0, 1 << 63)], 0, None, UNSUPPORTED),
        ("wires-one-short-dst", base, 0, 4, WIRE_OOB),
        ("wires-one-short-a", base + [INV(0, 4)], 0, 4, WIRE_OOB),
        ("wires-one-short-b", base + [XOR(0, 0, 5)], 0, 5, WIRE_OOB),
        ("inputs-above-wires", inputs(3), 0, 2, WIRE_OOB),
        ("outputs-above-wires", base, 6, None, WIRE_OOB),
        ("outputs-above-stated-wires", base, 9, 8, WIRE_OOB),
        ("outputs-above-empty", [], 1, None, WIRE_OOB),
        # pairs: the first in list order wins
        ("unsupported-then-bad", base + [op(SUB, 5, 0, 1), op(ADD, 6, 0, 1, reserved=1)], 0, None, UNSUPPORTED),
        ("bad-then-unsupported", base + [op(ADD, 5, 0, 1, reserved=1), op(SUB, 6, 0, 1)], 0, None, BAD_OP),
        ("oob-then-bad", base + [XOR(9, 0, 1), op(ADD, 6, 0, 1, reserved=1)], 0, 8, WIRE_OOB),
        ("bad-then-oob", base + [op(11, 5), XOR(9, 0, 1)], 0, 8, BAD_OP),
        ("oob-then-unsupported", base + [XOR(9, 0, 1), op(RANDOM, 5)], 0, 8, WIRE_OOB),
        # inside one record: BAD_OP before UNSUPPORTED before WIRE_OOB
        ("one-record-bad-unsupported-oob", base + [op(SUB, 99, 0, 1, domain=1, reserved=1)], 0, 8, BAD_OP),
        ("one-record-unsupported-oob", base + [op(SUB, 99, 0, 1)], 0, 8, UNSUPPORTED),
        ("one-record-imm-oob", base + [op(CONST, 99, 0, 0, 5)], 0, 8, UNSUPPORTED),
        # the fields a line does not name are not checked against n_wires
        ("records-before-header-check", base + [op(RANDOM, 5)], 99, None, UNSUPPORTED),
    ]
    return [(n, prog(p), o, w, c) for n, p, o, w, c in cases]


def want(program, n_outputs=0):
    """`dumps`' text, or None where it raises ValueError"""
    from reverie_amd import bristol

    try:
        return bristol.dumps(program, n_outputs)
    except ValueError:
        return None


def want_stated(program, n_outputs, n_wires):
    """the text for a stated wire count: `dumps`' with the header's second number replaced (None where dumps raises, or names an
    index at or above n_wires, or more outputs or inputs than n_wires)"""
    text = want(program, 0)
    if text is None:
        return None
    head, rest = text.split(b"\n", 1)
    gates, derived = head.split()
    n_in = int(rest.split(b"\n", 1)[0].split()[1])
    # (derived = the largest index named + 1, or the input count)
    if int(derived) > n_wires or n_outputs > n_wires or n_in > n_wires:
        return None
    return gates + b" %d\n1 %d\n1 %d\n\n" % (n_wires, n_in, n_outputs) + rest.split(b"\n\n", 1)[1]


def expect(program, n_outputs, n_wires):
    return want(program, n_outputs) if n_wires is None else want_stated(program, n_outputs, n_wires)


def derived(program):
    """(n_inputs, n_wires) of a list `dumps` writes, read off its header: what rv_bristol_writer_begin is told"""
    lines = want(program, 0).split(b"\n")
    return int(lines[1].split()[1]), int(lines[0].split()[1])


def fnv(data: bytes) -> int:
    h = 0xCBF29CE484222325
    for b in data:
        h = ((h ^ b) * 0x100000001B3) & 0xFFFFFFFFFFFFFFFF
    return h
