"""The op lists the pruning tests share (tests/test_prune_host.py, tests/test_gpu_prune.py), stated by intent: what is dead in each,
and which part of the device's order of work the shape goes around (the wavefront of 64, the workgroup of 256, the solo limit of
1 024, the emit tile of 256 records, the scans' tile of 2 048).  A case is (name, ops, wire counts, outputs_gf2, outputs_z64).
Deterministic."""
from __future__ import annotations

import numpy as np

import compact_cases
from reverie_amd.ops import B2A, GF2, OP_DTYPE, Z64, SizeHint, program

WAVE, WG, SOLO_LIMIT, TILE, SCAN_TILE = 64, 256, 1024, 256, 2048


def _prog(ops):
    return program(ops) if len(ops) else np.zeros(0, OP_DTYPE)


def _records(domain, opcode, dst, a, b):
    out = np.zeros(len(dst), OP_DTYPE)
    out["domain"], out["opcode"], out["dst"], out["a"], out["b"] = domain, opcode, dst, a, b
    return out


def dead_chain(depth, live=4):
    """a live head (an Input, `live` AddConsts, an assertion on the last) and behind it a chain of `depth` AddConsts nobody reads:
    `depth` frontier layers of width 1"""
    ops = [GF2.Input(0)] + [GF2.AddConst(1 + i, i, 1) for i in range(live)] + [GF2.AssertZero(live)]
    ops += [GF2.AddConst(live + 1 + i, live + i, i & 1) for i in range(depth)]
    return _prog(ops), (0, live + depth + 1)


def dead_layer(width):
    """`width` Muls of one Input, none read: one frontier layer of that width (the Input stays, unread)"""
    head = _prog([GF2.Input(0), GF2.Input(1), GF2.Add(2, 0, 1), GF2.AssertZero(2)])
    k = np.arange(width, dtype=np.uint32)
    return np.concatenate([head, _records(0, 6, 3 + k, 0, 1)]), (0, 3 + width)


def widen_narrow(levels=11):
    """a dead binary tree: its root is the first frontier, the layers double to 2^levels leaves (past the solo limit), every leaf
    reads ONE value twice, which is the next frontier alone, and a dead chain of 3 follows: 1, 2, .. 2^levels, 1, 1, 1, 1"""
    n_leaves = 1 << levels
    ops = [GF2.Input(0), GF2.AddConst(1, 0, 1), GF2.AddConst(2, 1, 1), GF2.AddConst(3, 2, 1), GF2.AddConst(4, 3, 0)]
    recs = [_prog(ops)]
    base = 5
    leaves = base + np.arange(n_leaves, dtype=np.uint32)
    recs.append(_records(0, 6, leaves, 4, 4))
    at, prev, width = base + n_leaves, leaves, n_leaves
    while width > 1:
        width //= 2
        dst = at + np.arange(width, dtype=np.uint32)
        recs.append(_records(0, 2, dst, prev[0::2], prev[1::2]))
        at, prev = at + width, dst
    recs.append(_prog([GF2.AssertZero(0)]))
    return np.concatenate(recs), (0, at)


def of_length(n, seed, n_idx=40):
    """exactly n ops over a few indices: every opcode of both domains, B2A and SizeHint now and then, few assertions, so that dead
    cones of every shape open"""
    rng = np.random.default_rng(seed)
    return random_list(rng, n, max(n_idx, 70), n_idx)


def random_list(rng, n, ng, nz):
    """n ops over ng GF(2) and nz Z64 indices (B2A only where 64 GF(2) indices exist) -> (ops, wire counts, outputs_gf2, outputs_z64)"""
    ops = np.zeros(n, OP_DTYPE)
    dom = (rng.random(n) < 0.4).astype(np.uint8)
    # few roots: Input 5 %, AssertZero 4 %; the rest spread over the other opcodes
    p = np.array([5, 6, 14, 10, 10, 8, 18, 8, 4, 8], float)
    opc = rng.choice(10, n, p=p / p.sum()).astype(np.uint8)
    lim = np.where(dom == 0, ng, nz)
    ops["domain"], ops["opcode"] = dom, opc
    for f in ("dst", "a", "b"):
        ops[f] = (rng.random(n) * lim).astype(np.uint32)
    ops["imm"] = rng.integers(0, 4, n)
    if ng >= 64 and nz >= 1:
        for i in np.flatnonzero(rng.random(n) < 0.02).tolist():
            ops[i] = B2A(int(rng.integers(0, nz)), int(rng.integers(0, ng - 63)))
    for i in np.flatnonzero(rng.random(n) < 0.01).tolist():
        ops[i] = SizeHint(int(rng.integers(0, nz + 1)), int(rng.integers(0, ng + 1)))
    outs_g = rng.integers(0, ng, int(rng.integers(0, 4))).astype(np.uint32).tolist()
    outs_z = rng.integers(0, nz, int(rng.integers(0, 3))).astype(np.uint32).tolist()
    return ops, (nz, ng), outs_g, outs_z


def generated(count=400):
    """the issue's generator: lists of 5 to 3 000 ops over 3 to 200 indices per domain"""
    out = []
    for s in range(count):
        rng = np.random.default_rng(7000 + s)
        n = int(rng.integers(5, 3001))
        ops, wc, og, oz = random_list(rng, n, int(rng.integers(3, 201)), int(rng.integers(3, 201)))
        out.append((f"generated_{s}", ops, wc, og, oz))
    return out


def b2a_cases():
    """live and dead B2As whose ranges overlap ([10, 73] live, [40, 103] dead), touch ([74, 137] dead) and stand apart; a dead B2A
    that is the only reader of the 64 values on [300, 363]; a live one that reads never-written indices ([200, 263])"""
    ops = [GF2.Input(0)]
    ops += [GF2.AddConst(10 + i, 0, i & 1) for i in range(128)]      # 10 .. 137: read by the live and the dead ranges
    ops += [GF2.AddConst(300 + i, 0, 1) for i in range(64)]          # read by the dead B2A alone
    ops += [B2A(0, 10), B2A(1, 40), B2A(2, 74), B2A(3, 300), B2A(4, 200), Z64.Add(5, 0, 4), Z64.Mul(6, 1, 2), Z64.AssertZero(5)]
    return _prog(ops), (8, 364)


def alignments():
    """tiles of 256 input records whose kept runs begin on an even and on an odd record of the output (an image at shift 0 and 8): tile
    0 keeps its Input alone, tile 1 all 256, tile 2 every other record, tile 3 the rest"""
    ops = [GF2.Input(0)] + [GF2.Mul(1 + i, 0, 0) for i in range(255)]
    ops += [GF2.Input(300 + i) for i in range(256)]
    for i in range(128):
        ops += [GF2.Input(600 + i), GF2.MulConst(800 + i, 600 + i, 1)]
    ops += [GF2.Add(1000, 300, 301), GF2.AssertZero(1000)] + [Z64.Random(i) for i in range(9)]
    return _prog(ops), (9, 1001)


def corpus():
    c = [("empty", _prog([]), (0, 0), [], [])]
    c.append(("all_live", _prog([GF2.Input(0), GF2.Input(1), GF2.Mul(2, 0, 1), GF2.Add(3, 2, 0), GF2.AssertZero(3), Z64.Input(0), Z64.Mul(1, 0, 0),
                                 Z64.SubConst(2, 1, 9), Z64.AssertZero(2)]), (3, 4), [], []))
    c.append(("inputs_alone_are_roots", _prog([GF2.Input(0), Z64.Input(0), GF2.Mul(1, 0, 0), Z64.Mul(1, 0, 0), GF2.Random(2), Z64.Const(2, 5),
                                               GF2.Add(3, 1, 2), Z64.Add(3, 1, 2)]), (4, 4), [], []))
    c.append(("dead_value_overwritten", _prog([GF2.Input(0), GF2.Mul(2, 0, 0), GF2.Add(2, 0, 0), GF2.AssertZero(2)]), (0, 3), [], []))
    c.append(("dead_overwrite_after_last_reader", _prog([GF2.Input(0), GF2.AddConst(1, 0, 1), GF2.AssertZero(1), GF2.Mul(1, 0, 0)]), (0, 2), [], []))
    c.append(("a_equals_b", _prog([GF2.Input(0), GF2.Mul(1, 0, 0), GF2.Mul(2, 1, 1), GF2.Add(3, 0, 0), GF2.AssertZero(3), Z64.Input(0),
                                   Z64.Mul(1, 0, 0), Z64.Sub(2, 1, 1)]), (3, 4), [], []))
    c.append(("never_written_reads", _prog([GF2.Add(0, 5, 6), GF2.Add(1, 7, 7), GF2.AssertZero(1), Z64.Mul(0, 3, 4), Z64.AssertZero(5),
                                            GF2.AssertZero(8)]), (6, 9), [], []))
    c.append(("output_nobody_writes", _prog([GF2.Input(0), GF2.Mul(1, 0, 0), Z64.Const(0, 1)]), (4, 12), [9, 1], [3]))
    c.append(("output_written_twice", _prog([GF2.Input(0), GF2.AddConst(1, 0, 1), GF2.Mul(2, 1, 1), GF2.AddConst(1, 0, 0), Z64.Const(2, 1),
                                             Z64.Const(2, 2)]), (3, 3), [1, 1], [2]))
    p, wc = b2a_cases()
    c.append(("b2a_ranges", p, wc, [], []))
    c.append(("b2a_output", p, wc, [300], [3, 6]))
    c.append(("dead_random_const_mulconst", _prog([GF2.Input(0), Z64.Input(0), GF2.Random(1), GF2.Const(2, 1), GF2.MulConst(3, 0, 1), Z64.Random(1),
                                                   Z64.Const(2, 7), Z64.MulConst(3, 0, 3), GF2.Random(4), GF2.AssertZero(4), Z64.Random(4),
                                                   Z64.MulConst(5, 4, 2), Z64.AssertZero(5)]), (6, 5), [], []))
    c.append(("sizehints_between_dropped", _prog([GF2.Input(0), GF2.Mul(1, 0, 0), SizeHint(2, 10), GF2.Mul(9, 1, 1), SizeHint(5, 80), Z64.Const(4, 1),
                                                  SizeHint(1, 1), B2A(3, 16), GF2.AssertZero(0)]), (0, 2), [], []))
    for depth in (1, 2, 5000):
        p, wc = dead_chain(depth)
        c.append((f"dead_chain_{depth}", p, wc, [], []))
    for width in (1, WAVE, WAVE + 1, WG, WG + 1, SOLO_LIMIT, SOLO_LIMIT + 1, 70000):
        p, wc = dead_layer(width)
        c.append((f"dead_layer_{width}", p, wc, [], []))
    p, wc = widen_narrow()
    c.append(("widen_past_solo_and_narrow", p, wc, [], []))
    for n in (1, TILE - 1, TILE, TILE + 1, SCAN_TILE - 1, SCAN_TILE, SCAN_TILE + 1, 70000):
        p, wc, og, oz = of_length(n, 31 + n)
        c.append((f"length_{n}", p, wc, og, oz))
    p, wc = alignments()
    c.append(("alignments", p, wc, [], []))
    # the wire compaction's corpus, pruned against its assertions (random and layered circuits, B2A ranges, SizeHints, sparse indices)
    for name, p, wc in compact_cases.generated() + compact_cases.edge_cases():
        c.append(("compact_" + name, p, wc, [], []))
    return c


def error_cases():
    """(name, ops, wire counts, outputs_gf2, outputs_z64, code or None: rv_ops_compact_wires' on the list)"""
    out = [(name, p, wc, [0], [1], None) for name, p, wc, _ in compact_cases.error_cases()]
    # two bad ops workgroups apart: the first in op order decides, whichever workgroup finishes first
    ok = [GF2.Input(i % 4) for i in range(700)]
    for name, first, second in (("bad_op_then_oob_far", (0, 11, 0, 0, 0, 0, 0), GF2.Add(4, 0, 1)), ("oob_then_bad_op_far", GF2.Add(4, 0, 1), (0, 11, 0, 0, 0, 0, 0))):
        ops = list(ok)
        ops[20], ops[650] = first, second
        out.append((name, _prog(ops), (2, 4), [], [], None))
    # an output index at the final count of its domain (a SizeHint raised it: 7 is inside, 8 is not)
    good = _prog([GF2.Input(0), SizeHint(3, 8), GF2.AssertZero(0)])
    out.append(("output_at_count_gf2", good, (2, 4), [7, 8], [], 9))
    out.append(("output_at_count_z64", good, (2, 4), [7], [3], 9))
    return out


def proof_programs():
    """small programs with dead Mul, B2A and Random for the proofs: (name, ops, wire counts, gf2 witness, z64 witness); every assertion
    holds for the witness, and fails when the witness's first entry is changed.  The GF(2) Mul and AssertZero counts are chosen so
    that the packed bit vectors of the proof are whole bytes before and after pruning (see test_prune_host.py for the layout)."""
    gf2 = [GF2.Input(0), GF2.Input(1)]
    for i in range(8):
        gf2 += [GF2.Mul(2 + i, 0, 1), GF2.Add(10 + i, 2 + i, 0), GF2.AddConst(10 + i, 10 + i, 1), GF2.AssertZero(10 + i)]  # in0 & in1 ^ in0 ^ 1
    gf2 += [GF2.Mul(20, 0, 1)] + [GF2.Mul(21 + i, 20 + i, 1) for i in range(14)] + [GF2.Random(40), GF2.Mul(41, 40, 34), GF2.Add(42, 41, 0)]
    z64 = [Z64.Input(0), Z64.Input(1), Z64.Mul(2, 0, 1), Z64.SubConst(3, 2, 15), Z64.AssertZero(3), Z64.Mul(4, 2, 2), Z64.Random(5), Z64.Mul(6, 5, 4),
           Z64.AddConst(7, 6, 1)]
    # wires 0 .. 62 are Inputs, wire 63 a live Mul of two more Inputs; the live B2A reads 0 .. 63 and its value is asserted
    mixed = [SizeHint(12, 140)] + [GF2.Input(i) for i in range(63)] + [GF2.Input(64), GF2.Input(65), GF2.Mul(63, 64, 65), B2A(0, 0),
                                                                     Z64.SubConst(1, 0, 5), Z64.AssertZero(1)]
    mixed += [GF2.Mul(66 + i, i, (i + 1) % 64) for i in range(64)] + [B2A(2, 66), Z64.Mul(3, 2, 0), GF2.Random(130), GF2.Mul(131, 130, 0), Z64.Random(4)]
    bits5 = [1, 0, 1] + [0] * 60 + [1, 0]
    return [("gf2", _prog(gf2), (0, 43), [1, 0], []), ("z64", _prog(z64), (8, 0), [], [3, 5]), ("mixed", _prog(mixed), (12, 140), bits5, [])]
