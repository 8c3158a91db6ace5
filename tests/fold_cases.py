"""The op lists the folding tests share (tests/test_fold_host.py, tests/test_gpu_fold.py), stated by intent: what is known in each,
and which part of the device's order of work the shape goes around (the wavefront of 64, the workgroup of 256, the solo limit, the
rewrite tile of 256 records).  A case is (name, ops, wire counts (z64, gf2)).  Deterministic."""
from __future__ import annotations

import numpy as np

import compact_cases
from reverie_amd.ops import B2A, GF2, OP_DTYPE, Z64, SizeHint, program

WAVE, WG, TILE = 64, 256, 256
M64 = (1 << 64) - 1


def _prog(ops):
    return program(ops) if len(ops) else np.zeros(0, OP_DTYPE)


def _records(domain, opcode, dst, a=0, b=0, imm=0):
    out = np.zeros(len(dst), OP_DTYPE)
    out["domain"], out["opcode"], out["dst"], out["a"], out["b"], out["imm"] = domain, opcode, dst, a, b, imm
    return out


def known_chain(depth):
    """an Input, then a Z64 Const and `depth - 1` linear ops each of the one before (the layers: 1 wide, `depth` of them), a Mul of
    the chain's end with the Input (it becomes a MulConst) and an assertion on it"""
    ops = [Z64.Input(0), Z64.Const(1, 3)]
    for i in range(1, depth):
        ops.append((Z64.AddConst, Z64.MulConst, Z64.SubConst)[i % 3](1 + i, i, 2 * i + 1))
    ops += [Z64.Mul(depth + 1, 0, depth), Z64.AssertZero(depth + 1)]
    return _prog(ops), (depth + 2, 0)


def known_layer(width):
    """a GF(2) Const, `width` AddConsts of it (the layers: 1, then `width` wide), and an Add of each with an Input (an AddConst
    afterwards)"""
    k = np.arange(width, dtype=np.uint32)
    recs = [_prog([GF2.Input(0), GF2.Const(1, 1)]), _records(0, 3, 2 + k, 1, 0, k & 1), _records(0, 2, 2 + width + k, 0, 2 + k),
            _prog([GF2.AssertZero(2 + width)])]
    return np.concatenate(recs), (0, 2 + 2 * width)


def widen_narrow(levels=11):
    """a known binary tree that fans out from one Const to 2^levels AddConsts (past the solo limit) and is then summed pairwise back
    to one value: the layers are 1, 2, .. 2^levels, 2^(levels-1), .. 1 wide; the root is multiplied with an Input"""
    recs = [_prog([Z64.Input(0), Z64.Const(1, 1)])]
    prev, at = np.array([1], np.uint32), 2
    for _ in range(levels):
        dst = at + np.arange(2 * len(prev), dtype=np.uint32)
        recs.append(_records(1, 3, dst, np.repeat(prev, 2), 0, dst.astype(np.uint64) * 0x9E3779B97F4A7C15))
        prev, at = dst, at + len(dst)
    while len(prev) > 1:
        dst = at + np.arange(len(prev) // 2, dtype=np.uint32)
        recs.append(_records(1, 2, dst, prev[0::2], prev[1::2]))
        prev, at = dst, at + len(dst)
    recs.append(_prog([Z64.Mul(at, 0, int(prev[0])), Z64.AssertZero(at)]))
    return np.concatenate(recs), (at + 1, 0)


# the opcode mix of the random lists: Input, Random, Add, AddConst, Sub, SubConst, Mul, MulConst, AssertZero, Const
MIX = np.array([10, 4, 14, 9, 12, 8, 18, 9, 5, 11], float)


def random_list(rng, n, ng=70, nz=40, consts=True, written=0.0):
    """n ops over ng GF(2) and nz Z64 indices, like prune_cases.random_list with Const and zero MulConst mixed in (imm 0 .. 3: half
    of the GF(2) MulConsts and a quarter of the Z64 ones are zero).  consts False: no Const and no zero MulConst; written: the
    fraction of the indices of both domains that an Input writes first (1.0: no read finds an unwritten index)."""
    head = [GF2.Input(i) for i in range(ng) if rng.random() < written] + [Z64.Input(i) for i in range(nz) if rng.random() < written]
    ops = np.zeros(n, OP_DTYPE)
    dom = (rng.random(n) < 0.4).astype(np.uint8)
    p = MIX.copy()
    if not consts:
        p[9] = 0
    opc = rng.choice(10, n, p=p / p.sum()).astype(np.uint8)
    lim = np.where(dom == 0, ng, nz)
    ops["domain"], ops["opcode"] = dom, opc
    for f in ("dst", "a", "b"):
        ops[f] = (rng.random(n) * lim).astype(np.uint32)
    ops["imm"] = rng.integers(0, 4, n)
    if not consts:
        ops["imm"][opc == 7] |= 1
    if ng >= 64 and nz >= 1:
        for i in np.flatnonzero(rng.random(n) < 0.03).tolist():
            ops[i] = B2A(int(rng.integers(0, nz)), int(rng.integers(0, ng - 63)))
    for i in np.flatnonzero(rng.random(n) < 0.01).tolist():
        ops[i] = SizeHint(int(rng.integers(0, nz + 1)), int(rng.integers(0, ng + 1)))
    return np.concatenate([_prog(head), ops]), (nz, ng)


def generated(count=400):
    """the issue's generator: lists of 1 to 300 random ops (behind the Inputs that write indices first, up to 110 of them) over about
    40 indices (70 GF(2) ones, so that a B2A fits).  Every fifth list has
    every index written by an Input first and no constants -- nothing is known in it; the others have a random share of their
    indices written first, and every other one of them writes most GF(2) values as constants, so that whole B2A ranges are known."""
    out = []
    for s in range(count):
        rng = np.random.default_rng(9000 + s)
        n = int(rng.integers(1, 301))
        if s % 5 == 0:
            ops, wc = random_list(rng, n, consts=False, written=1.0)
        else:
            ops, wc = random_list(rng, n, written=float(rng.random()) * (s % 2))
            if s % 2:
                g = np.flatnonzero((ops["domain"] == 0) & (ops["opcode"] != 8) & (rng.random(len(ops)) < 0.6))
                ops["opcode"][g] = 9
        out.append((f"generated_{s}", ops, wc))
    return out


def of_length(n, seed):
    ops, wc = random_list(np.random.default_rng(seed), n)
    return ops[:n], wc


def single_kinds():
    """each rewrite kind alone, in both domains: (name, ops, wire counts).  Wire 0 is an Input x, wire 1 a Const c (GF(2): 1; Z64: 6),
    wire 2 a Const 0."""
    out = []
    for t, D, c in (("g", GF2, 1), ("z", Z64, 6)):
        head = [D.Input(0), D.Const(1, c), D.Const(2, 0)]
        wc = (0, 8) if D is GF2 else (8, 0)
        for name, ops in (("mul_const", [D.Mul(3, 1, 1)]), ("mul_linear_a", [D.Mul(3, 1, 0)]), ("mul_linear_b", [D.Mul(3, 0, 1)]),
                          ("add_addconst_a", [D.Add(3, 1, 0)]), ("add_addconst_b", [D.Add(3, 0, 1)]), ("sub_subconst", [D.Sub(3, 0, 1)]),
                          ("sub_a_known", [D.Sub(3, 1, 0)]), ("add_const", [D.Add(3, 1, 2)]), ("sub_const", [D.Sub(3, 2, 1)]),
                          ("addconst_const", [D.AddConst(3, 1, 3)]), ("subconst_const", [D.SubConst(3, 2, 3)]), ("mulconst_const", [D.MulConst(3, 1, 3)]),
                          ("zero_mulconst", [D.MulConst(3, 0, 0 if D is Z64 else 2)]), ("mul_zero_a", [D.Mul(3, 2, 0)]), ("mul_zero_b", [D.Mul(3, 0, 2)]),
                          ("mul_x_x_known", [D.Mul(3, 1, 1), D.Mul(4, 2, 2)]), ("mul_x_x_unknown", [D.Mul(3, 0, 0)]),
                          ("assert_known_zero", [D.AssertZero(2)]), ("assert_known_nonzero", [D.AssertZero(1)]), ("assert_unknown", [D.AssertZero(0)])):
            out.append((f"{t}_{name}", _prog(head + ops + [D.AssertZero(3)]), wc))
    return out


def b2a_cases():
    """B2As over 64 known bits (Consts and unwritten indices), 63 known bits with the unknown one first and last, no known bit"""
    bits = [(0x8000000000000005 >> k) & 1 for k in range(64)]
    out = []
    for name, unknown in (("b2a_64_known", ()), ("b2a_63_known_first_unknown", (0,)), ("b2a_63_known_last_unknown", (63,)), ("b2a_0_known", range(64))):
        ops = [GF2.Input(100)]
        ops += [GF2.AddConst(k, 100, 1) if k in unknown else GF2.Const(k, bits[k] | 2) for k in range(64) if k % 7 != 3 or k in unknown]  # (k % 7 == 3: unwritten)
        ops += [B2A(0, 0), Z64.Input(1), Z64.Mul(2, 0, 1), Z64.AssertZero(2)]
        out.append((name, _prog(ops), (3, 101)))
    return out


def corpus(solo_limit=1024):
    """solo_limit: rv_hook_fold_limits' second word (the tests read it)"""
    c = [("empty", _prog([]), (0, 0)), ("one_const", _prog([GF2.Const(0, 1)]), (0, 1)), ("one_input", _prog([Z64.Input(0)]), (1, 0))]
    c += single_kinds()
    c.append(("z64_wrap", _prog([Z64.Input(0), Z64.Const(1, 1 << 63), Z64.Const(2, M64), Z64.Const(3, 5), Z64.Sub(4, 3, 2), Z64.Sub(5, 3, 1),
                                 Z64.MulConst(6, 1, 2), Z64.MulConst(7, 2, M64), Z64.Mul(8, 1, 1), Z64.Mul(9, 2, 2), Z64.Mul(10, 2, 1), Z64.Mul(11, 0, 2),
                                 Z64.Mul(12, 1, 0), Z64.SubConst(13, 3, 9), Z64.AddConst(14, 2, 1), Z64.Add(15, 2, 2), Z64.AssertZero(14)]), (16, 0)))
    c.append(("gf2_const_high_bits", _prog([GF2.Input(0), GF2.Const(1, 0xFFFFFFFFFFFFFFFE), GF2.Const(2, 0xFFFFFFFFFFFFFFFF), GF2.Mul(3, 0, 1), GF2.Mul(4, 0, 2),
                                            GF2.Add(5, 0, 2), GF2.AddConst(6, 1, 0xFFFFFFFFFFFFFFFF), GF2.MulConst(7, 0, 0xFFFFFFFFFFFFFFFE)]), (0, 8)))
    c.append(("mul_zero_other_input", _prog([GF2.Input(0), GF2.Const(1, 0), GF2.Mul(2, 0, 1), GF2.Mul(3, 1, 0), GF2.AssertZero(2), Z64.Input(0), Z64.Const(1, 0),
                                             Z64.Mul(2, 0, 1), Z64.Mul(3, 1, 0), Z64.AssertZero(3)]), (4, 4)))
    c.append(("unwritten_reads", _prog([GF2.Input(0), GF2.Add(1, 9, 0), GF2.Add(2, 0, 9), GF2.Mul(3, 9, 0), GF2.Sub(4, 9, 0), GF2.Add(5, 8, 9), GF2.AssertZero(9),
                                        Z64.Input(0), Z64.Sub(1, 9, 0), Z64.Sub(2, 0, 9), Z64.Mul(3, 0, 9), Z64.AddConst(4, 9, 7), Z64.AssertZero(4)]), (10, 10)))
    c.append(("unwritten_in_b2a_range", _prog([GF2.Const(3, 1), GF2.Const(40, 1), B2A(0, 0), Z64.Input(1), Z64.Mul(2, 0, 1), GF2.Input(70), B2A(3, 10),
                                               Z64.Add(4, 3, 0)]), (5, 80)))
    c.append(("known_then_unknown", _prog([GF2.Input(0), GF2.Const(1, 1), GF2.Mul(2, 0, 1), GF2.Add(1, 0, 0), GF2.Mul(3, 0, 1), GF2.Const(1, 0), GF2.Mul(4, 0, 1),
                                           GF2.Input(1), GF2.Mul(5, 0, 1), Z64.Input(0), Z64.Const(1, 4), Z64.Add(2, 0, 1), Z64.Input(1), Z64.Add(3, 0, 1)]), (4, 6)))
    c.append(("unknown_then_known", _prog([Z64.Input(0), Z64.Input(1), Z64.Mul(2, 0, 1), Z64.Const(1, 9), Z64.Mul(3, 0, 1), Z64.Mul(1, 1, 1), Z64.Mul(4, 0, 1),
                                           Z64.Sub(0, 1, 1), Z64.Mul(5, 0, 0), GF2.Input(0), GF2.Add(0, 0, 0), GF2.Const(0, 1), GF2.Add(1, 0, 0)]), (6, 2)))
    c += b2a_cases()
    c.append(("sizehint_grows", _prog([GF2.Const(0, 1), SizeHint(2, 10), GF2.Add(9, 0, 0), Z64.Input(1), SizeHint(1, 4), SizeHint(5, 80), Z64.Add(4, 1, 3),
                                       B2A(2, 16), Z64.Mul(3, 2, 1), GF2.AssertZero(9)]), (0, 1)))
    ops, wc = random_list(np.random.default_rng(5), 600, consts=False, written=1.0)
    c.append(("nothing_known", ops, wc))
    for depth in (1, 2, 63, 64, 65, 3000):
        p, wc = known_chain(depth)
        c.append((f"known_chain_{depth}", p, wc))
    for width in (1, WAVE, WAVE + 1, WG + 1, solo_limit - 1, solo_limit, solo_limit + 1):
        p, wc = known_layer(width)
        c.append((f"known_layer_{width}", p, wc))
    p, wc = widen_narrow()
    c.append(("widen_past_solo_and_narrow", p, wc))
    for n in (TILE - 1, TILE, TILE + 1, 2 * TILE + 1):
        p, wc = of_length(n, 77 + n)
        c.append((f"length_{n}", p, wc))
    # the wire compaction's edge cases (sparse indices, B2A ranges, SizeHints, reads of unwritten indices)
    for name, p, wc in compact_cases.edge_cases():
        c.append(("compact_" + name, p, wc))
    return c


def error_cases():
    """(name, ops, wire counts): prune's -- a bad opcode, reserved != 0, an index out of bounds before and after a SizeHint, a B2A
    range over the end -- and two bad ops workgroups apart (the first in op order decides)"""
    out = [(name, p, wc) for name, p, wc, _ in compact_cases.error_cases()]
    ok = [GF2.Const(i % 4, i & 1) for i in range(700)]
    for name, first, second in (("bad_op_then_oob_far", (0, 11, 0, 0, 0, 0, 0), GF2.Add(4, 0, 1)), ("oob_then_bad_op_far", GF2.Add(4, 0, 1), (0, 11, 0, 0, 0, 0, 0))):
        ops = list(ok)
        ops[20], ops[650] = first, second
        out.append((name, _prog(ops), (2, 4)))
    return out


def proof_programs():
    """small programs with Muls and a B2A that fold away, for the proofs: (name, ops, wire counts, gf2 witness, z64 witness, the folded
    (GF(2) Mul, Z64 Mul, B2A) counts).  Every assertion holds for the witness.  The counts keep the packed bit vectors of the proof
    whole bytes before and after folding, and after the pruning that follows (test_prune_host.py has the layout); in each program
    Muls that cannot be folded are read by a Mul with a known 0 alone, so that pruning the folded list drops them."""
    gf2 = [GF2.Input(0), GF2.Input(1), GF2.Const(2, 1), GF2.Const(3, 0)]
    for i in range(8):
        gf2 += [GF2.Mul(10 + i, 0, 1), GF2.Add(20 + i, 10 + i, 0), GF2.AddConst(20 + i, 20 + i, 1), GF2.AssertZero(20 + i)]  # in0 & in1 ^ in0 ^ 1
    gf2 += [GF2.Mul(30 + i, 0, 1) for i in range(8)] + [GF2.Mul(40 + i, 30 + i, 3) for i in range(8)]  # 8 stay, 8 are 0
    gf2 += [GF2.Mul(50 + i, i & 1, 2) for i in range(4)] + [GF2.Mul(54 + i, 2, 2 + (i & 1)) for i in range(4)]  # 4 linear, 4 constant
    z64 = [Z64.Input(0), Z64.Input(1), Z64.Mul(2, 0, 1), Z64.SubConst(3, 2, 15), Z64.AssertZero(3), Z64.Const(4, 7), Z64.Mul(5, 0, 4), Z64.Const(6, 0),
           Z64.Mul(7, 2, 2), Z64.Mul(8, 7, 6)]
    bits = [(0xC3A5 >> (k % 16)) & 1 for k in range(64)]
    mixed = [SizeHint(12, 300)] + [GF2.Input(i) for i in range(63)] + [GF2.Input(64), GF2.Input(65), GF2.Mul(63, 64, 65), B2A(0, 0), Z64.SubConst(1, 0, 5),
                                                                     Z64.AssertZero(1)]
    mixed += [GF2.Const(200 + k, bits[k]) for k in range(64)] + [B2A(2, 200), Z64.Mul(3, 2, 0)]  # a B2A of 64 known bits, a Mul by its value
    mixed += [GF2.Const(130, 1), GF2.Const(129, 0)] + [GF2.Mul(131 + i, i, 130) for i in range(56)] + [GF2.Mul(187 + i, 130, 129 + (i & 1)) for i in range(8)]
    mixed += [GF2.Mul(270 + i, i, i + 1) for i in range(8)] + [GF2.Add(280, 270, 271)] + [GF2.Add(280, 280, 272 + i) for i in range(6)] + [GF2.Mul(281, 280, 129)]
    bits5 = [1, 0, 1] + [0] * 60 + [1, 0]
    return [("gf2", _prog(gf2), (0, 64), [1, 0], [], (16, 0, 0)), ("z64", _prog(z64), (9, 0), [], [3, 5], (0, 2, 0)),
            ("mixed", _prog(mixed), (12, 300), bits5, [], (65, 1, 1))]
