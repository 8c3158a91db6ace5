"""The op lists the wire-compaction tests share (tests/test_compact_wires_host.py, tests/test_gpu_compact_wires.py): the corpus the
host sweep and the device kernels are compared on with tests/compact_ref.py, and the lists with errors in them.  Deterministic."""
from __future__ import annotations

import json
import os

import numpy as np

import circuits
from reverie_amd.ops import B2A, GF2, OP_DTYPE, Z64, SizeHint, program

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
TILE = 2048  # ops one workgroup of the device scans covers (csrc/compact_dev.h: COMPACT_TILE)


def _prog(ops):
    return program(ops) if len(ops) else np.zeros(0, OP_DTYPE)


def golden():
    from conftest import golden_ops

    meta = json.load(open(os.path.join(GOLDEN, "proofs.json")))
    return [("golden_" + name, _prog(golden_ops(m)), tuple(m["wire_counts"])) for name, m in sorted(meta.items())]


def chain(depth):
    """Add(w_{i+1}, w_i, w_i): every value takes its predecessor's slot one op late -- a reuse chain `depth` long"""
    return _prog([GF2.Input(0)] + [GF2.Add(i + 1, i, i) for i in range(depth)] + [GF2.AssertZero(depth)]), (0, depth + 1)


def of_length(n, seed):
    """exactly n ops: GF(2) and Z64 ops over a few wires, every kind of read (both domains interleaved)"""
    rng = np.random.default_rng(seed)
    kind = rng.integers(0, 8, n)
    w = rng.integers(0, 24, (n, 3))
    ops = []
    for k, (d, a, b) in zip(kind.tolist(), w.tolist()):
        ops.append((GF2.Input(d), GF2.Mul(d, a, b), GF2.Add(d, a, a), GF2.AssertZero(a), Z64.Const(d, 7), Z64.Mul(d, a, b),
                    Z64.AddConst(d, a, 3), Z64.AssertZero(a))[k])
    return _prog(ops), (24, 24)


def edge_cases():
    out = [("empty", _prog([]), (0, 0)), ("one_input", _prog([GF2.Input(5)]), (0, 9)), ("one_assert", _prog([Z64.AssertZero(3)]), (4, 0))]
    k = 300
    # no value is released before the last defining op: every slot is fresh
    out.append(("all_fresh", _prog([GF2.Input(i) for i in range(k)] + [GF2.AssertZero(k - 1 - i) for i in range(k)]), (0, k)))
    # only dead values: each is released by the op that defines it
    out.append(("all_dead", _prog([GF2.Const(i, i & 1) for i in range(k)] + [Z64.Input(2 * i) for i in range(k)]), (2 * k, k)))
    out.append(("a_equals_b", _prog([GF2.Input(0), GF2.Input(1), GF2.Mul(2, 0, 0), GF2.Add(3, 1, 1), GF2.Mul(4, 2, 3), GF2.Mul(5, 4, 4),
                                     Z64.Input(0), Z64.Mul(1, 0, 0), Z64.Sub(2, 1, 1), Z64.AssertZero(2)]), (3, 6)))
    out.append(("assert_last_reader", _prog([GF2.Input(0), GF2.AddConst(1, 0, 1), GF2.AssertZero(1), GF2.Input(2), GF2.AssertZero(0),
                                             GF2.Input(3), GF2.Mul(4, 2, 3), GF2.AssertZero(4)]), (0, 5)))
    big = (1 << 24) + 5
    out.append(("sparse", _prog([GF2.Input(big), GF2.Input(7), GF2.Mul(1 << 20, big, 7), GF2.Add((1 << 16) + 1, 1 << 20, 255), GF2.AssertZero((1 << 16) + 1),
                                 Z64.Input(big), Z64.Mul(1 << 23, big, 256), Z64.AssertZero(1 << 23)]), (big + 1, big + 1)))
    # B2A ranges that overlap ([10, 73] and [40, 103]), touch ([104, 167]) and stand apart ([300, 363]); pinned indices written, read
    # before they are written (12, 13) and never written; indices between and behind the ranges in the pool
    ops = [GF2.Add(200, 12, 13), GF2.Input(5)]
    ops += [GF2.AddConst(10 + i, 5, i & 1) for i in range(0, 94, 3)]
    ops += [B2A(0, 10), GF2.Input(250), GF2.Mul(251, 250, 20), B2A(1, 40), GF2.AddConst(104, 251, 1), B2A(2, 104), GF2.Mul(9, 5, 168),
            B2A(3, 300), Z64.Add(4, 0, 1), Z64.Mul(0, 2, 3), Z64.Sub(5, 4, 7), GF2.Add(301, 9, 200), B2A(1, 300)]
    out.append(("b2a_ranges", _prog(ops), (8, 364)))
    # SizeHints that grow the counts mid-list (and one that grows nothing)
    out.append(("sizehints", _prog([GF2.Input(0), SizeHint(2, 10), GF2.Add(9, 0, 0), Z64.Input(1), SizeHint(1, 4), SizeHint(5, 80), Z64.Add(4, 1, 3),
                                    B2A(2, 16), GF2.AssertZero(9)]), (0, 1)))
    out.append(("zero_reads", _prog([GF2.Add(0, 1, 2), Z64.Add(0, 1, 2), GF2.AssertZero(3), Z64.Mul(1, 0, 9)]), (10, 4)))
    p, c = chain(40)
    out.append(("chain40", p, c))
    return out


def generated():
    out = []
    for s in range(20):
        p, _, c = circuits.random_gf2(np.random.default_rng(s), n_wires=3 + 3 * s)
        out.append((f"random_gf2_{s}", p, c))
    for s in range(10):
        p, _, _, c = circuits.random_mixed(np.random.default_rng(100 + s))
        out.append((f"random_mixed_{s}", p, c))
    for recycle in (False, True):
        p, _, c, _ = circuits.layered_gf2(n_in=64, width=256, layers=12, fold_to=16, recycle=recycle)
        out.append((f"layered_gf2_{'recycled' if recycle else 'ssa'}", p, c))
        p, _, c, _ = circuits.layered_z64(n_in=16, width=64, n_mul=300, recycle=recycle)
        out.append((f"layered_z64_{'recycled' if recycle else 'ssa'}", p, c))
    return out


def corpus():
    return golden() + generated() + edge_cases()


def error_cases():
    """(name, ops, wire counts, the code where the oracle cannot give it or None): each list has an op the compiler refuses"""
    ok = [GF2.Const(0, 1), GF2.Const(1, 0), GF2.Mul(2, 0, 1), Z64.Const(0, 5), Z64.Add(1, 0, 0), GF2.AssertZero(3)]
    wc = (2, 4)

    def at(i, op):
        ops = list(ok)
        ops.insert(i, op)
        return _prog(ops)

    bad_reserved = at(2, GF2.Add(3, 0, 1))
    bad_reserved["reserved"][2] = 1
    hint_reserved = at(2, SizeHint(2, 4))
    hint_reserved["reserved"][2] = 7
    return [
        ("bad_opcode", at(3, (0, 10, 0, 1, 0, 0, 0)), wc, None),
        ("bad_opcode_z64", at(3, (1, 200, 0, 1, 0, 0, 0)), wc, None),
        ("bad_domain", at(1, (4, 2, 0, 1, 0, 0, 0)), wc, None),
        ("reserved", bad_reserved, wc, 5),
        ("reserved_sizehint", hint_reserved, wc, 5),
        ("dst_at_count", at(4, GF2.Add(4, 0, 1)), wc, None),
        ("a_at_count", at(4, GF2.AddConst(0, 4, 1)), wc, None),
        ("b_at_count", at(4, Z64.Mul(0, 1, 2)), wc, None),
        ("assert_at_count", at(6, Z64.AssertZero(2)), wc, None),
        ("b2a_src_short", at(3, B2A(0, 0)), wc, None),
        ("b2a_dst", _prog([SizeHint(2, 70), B2A(2, 0)]), wc, None),
        ("legal_after_later_hint", _prog(ok + [GF2.Add(5, 0, 1), SizeHint(2, 8)]), wc, None),
        ("hint_then_beyond", _prog([SizeHint(2, 8)] + ok + [GF2.Add(8, 0, 1)]), wc, None),
        ("oob_then_bad_op", _prog(ok + [GF2.Add(4, 0, 1), (0, 11, 0, 0, 0, 0, 0)]), wc, None),
        ("bad_op_then_oob", _prog(ok + [(0, 11, 0, 0, 0, 0, 0), GF2.Add(4, 0, 1)]), wc, None),
    ]


def oracle_code(oracle, prog, wc):
    """the code the compiler gives for the list, through the oracle (which steps the list as the reference does): 0 for a good one"""
    try:
        oracle.prove(prog, [], [], wc, np.zeros((256, 16), np.uint8))
    except oracle.OracleError as e:
        return e.code
    return 0
