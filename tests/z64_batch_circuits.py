"""Z64 circuits for the batched prover / verifier (tests/test_gpu_batch_z64.py, tools/batch_z64.py)."""
import numpy as np

import circuits
from reverie_amd.ops import Z64, largest_wires, program

MASK64 = (1 << 64) - 1


def chain_z64(lanes=4, rounds=128, seed=7):
    """`lanes` independent chains x <- x*x + c for `rounds` rounds, final values asserted: a deep, narrow pure-Z64 circuit
    in which every dependency level holds Z64 gates (a Mul level, then an AddConst level, per round).
    -> (program, z64 witness, wire_counts)"""
    rng = np.random.default_rng(seed)
    wit = [int(v) for v in rng.integers(0, 1 << 63, lanes, dtype=np.uint64)]
    consts = [int(v) for v in rng.integers(1, 1 << 62, lanes, dtype=np.uint64)]
    ops = [Z64.Input(i) for i in range(lanes)]
    cur = list(range(lanes))
    vals = list(wit)
    pos = lanes
    for _ in range(rounds):
        for k in range(lanes):
            ops.append(Z64.Mul(pos, cur[k], cur[k]))
            ops.append(Z64.AddConst(pos + 1, pos, consts[k]))
            vals[k] = (vals[k] * vals[k] + consts[k]) & MASK64
            cur[k] = pos + 1
            pos += 2
    for k in range(lanes):
        ops.append(Z64.SubConst(pos, cur[k], vals[k]))
        ops.append(Z64.AssertZero(pos))
        pos += 1
    prog = program(ops)
    return prog, wit, largest_wires(prog)


def random_gates_z64(n_in=6, n_gates=300, seed=3):
    """Z64 gates of every kind including Random; only wires whose clear value does not depend on a Random gate are
    asserted.  -> (program, z64 witness, wire_counts)"""
    rng = np.random.default_rng(seed)
    wit = [int(v) for v in rng.integers(0, 1 << 63, n_in, dtype=np.uint64)]
    ops = [Z64.Input(i) for i in range(n_in)]
    vals = list(wit)  # None: depends on a Random gate
    for _ in range(n_gates):
        d = len(vals)
        a, b = int(rng.integers(0, d)), int(rng.integers(0, d))
        k = int(rng.integers(0, 8))
        c = int(rng.integers(0, 1 << 63))
        va, vb = vals[a], vals[b]
        known = va is not None and vb is not None
        if k == 0:
            ops.append(Z64.Random(d)); v = None
        elif k == 1:
            ops.append(Z64.Mul(d, a, b)); v = (va * vb) & MASK64 if known else None
        elif k == 2:
            ops.append(Z64.Add(d, a, b)); v = (va + vb) & MASK64 if known else None
        elif k == 3:
            ops.append(Z64.Sub(d, a, b)); v = (va - vb) & MASK64 if known else None
        elif k == 4:
            ops.append(Z64.MulConst(d, a, c)); v = (va * c) & MASK64 if va is not None else None
        elif k == 5:
            ops.append(Z64.AddConst(d, a, c)); v = (va + c) & MASK64 if va is not None else None
        elif k == 6:
            ops.append(Z64.Const(d, c)); v = c
        else:
            ops.append(Z64.Mul(d, a, a)); v = (va * va) & MASK64 if va is not None else None
        vals.append(v)
    for w in range(n_in, len(vals), 7):
        if vals[w] is not None:
            d = len(vals)
            ops.append(Z64.SubConst(d, w, vals[w]))
            ops.append(Z64.AssertZero(d))
            vals.append(0)
    prog = program(ops)
    return prog, wit, largest_wires(prog)


def layered_small(n_mul=10_000):
    """a small circuits.layered_z64 (~n_mul Mul gates).  -> (program, z64 witness, wire_counts)"""
    prog, wit, wc, _ = circuits.layered_z64(n_in=256, width=2048, n_mul=n_mul)
    return prog, wit, wc


def mixed(seed, n_gates=200):
    """circuits.random_mixed (B2A, Random, SizeHint).  -> (program, gf2 witness, z64 witness, wire_counts)"""
    return circuits.random_mixed(np.random.default_rng(seed), n_gates=n_gates)
