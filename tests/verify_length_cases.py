"""The circuits of the altered-vector-length tests (tests/proof_mutate.py), their oracle proofs, catalogues and the
oracle's answers -- shared by test_proof_mutate_host.py (CPU) and test_gpu_verify_lengths.py.  TEST INFRASTRUCTURE.

    MIX   GF(2) + Z64, the general verifier path: 600 GF(2) and 3 Z64 inputs, 5000 GF(2) Mul/Add gates on 24 reused wires, a Z64
          Mul behind every 11th, valid AssertZero gates in both domains
    WIDE  pure GF(2), wide levels, one base per wire: the compact-corrections verifier
    Z     pure Z64: the fused Z64 verifier below its quad-group split.  layered_z64(64, 256, 1500) is the shape
          tests/test_gpu_z64_fused.py::test_fused_invalid_witness_and_reuse proves on the fused path; the GPU test checks the
          eligibility through the circuit's device bytes
    SPLIT pure Z64 with more than 4 MiB of online records (split_circuit, GPU test only, reduced catalogue): the fused Z64
          verifier's quad-group split, which the proof's copy on the side stream switches on

GF(2) vector lengths: 600 inputs are an `in` vector of 76 bytes, two 64-byte unpack tiles, so the cuts to 127 / 128 / 129 bytes
do not exist for `in`; they are made on `corr` and `rec` (MIX: 417 / 418 bytes, seven tiles; WIDE: 125 / 189 bytes, where only
`rec` reaches them).
"""
from __future__ import annotations

import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np

import circuits
import proof_mutate
from reverie_amd.ops import GF2, Z64, program

NAMES = ("MIX", "WIDE", "Z")
M64 = (1 << 64) - 1


def mix_circuit():
    rng = np.random.default_rng(0x4C454E)
    n_in, n_work = 600, 24
    scratch2, scratch64 = n_in + n_work, 8
    w2 = rng.integers(0, 2, n_in).tolist()
    w64 = [int(x) for x in rng.integers(0, 1 << 63, 3, dtype=np.uint64)]
    v2 = w2 + [0] * (n_work + 1)
    v64 = w64 + [0] * 6
    ops = [GF2.Input(i) for i in range(n_in)] + [Z64.Input(i) for i in range(3)]

    def operand():
        return int(rng.integers(n_in, n_in + n_work)) if rng.random() < 0.7 else int(rng.integers(0, n_in))

    def asserts():
        a = operand()
        ops.append(GF2.AddConst(scratch2, a, v2[a]))
        ops.append(GF2.AssertZero(scratch2))
        b = int(rng.integers(0, 8))
        ops.append(Z64.SubConst(scratch64, b, v64[b]))
        ops.append(Z64.AssertZero(scratch64))

    for i in range(5000):
        a, b, d = operand(), operand(), int(rng.integers(n_in, n_in + n_work))
        if i % 3:
            ops.append(GF2.Mul(d, a, b))
            v2[d] = v2[a] & v2[b]
        else:
            ops.append(GF2.Add(d, a, b))
            v2[d] = v2[a] ^ v2[b]
        if i % 11 == 0:
            d, a, b = int(rng.integers(3, 8)), int(rng.integers(0, 8)), int(rng.integers(0, 8))
            ops.append(Z64.Mul(d, a, b))
            v64[d] = (v64[a] * v64[b]) & M64
        if i in (1700, 3400):
            asserts()
    for _ in range(3):
        asserts()
    return program(ops), w2, w64, (scratch64 + 1, scratch2 + 1)


def circuit(name):
    """-> (prog, wit_gf2, wit_z64, wire_counts)"""
    if name == "MIX":
        return mix_circuit()
    if name == "WIDE":
        prog, wit, wc, _ = circuits.layered_gf2(n_in=600, width=512, layers=4, fold_to=512)
        return prog, list(wit), [], wc
    if name == "Z":
        prog, wit, wc, _ = circuits.layered_z64(n_in=64, width=256, n_mul=1500)
        return prog, [], wit, wc
    raise KeyError(name)


def split_circuit():
    """-> (prog, wit_z64, wire_counts): 7400 Z64 Mul gates, 40 x (16 x 7400 + ...) bytes = 4.8 MB of online records -- above the
    4 MiB from which the verifier copies the proof on its second stream, even with one group's `rec` or `corr` emptied"""
    prog, wit, wc, _ = circuits.layered_z64(n_in=64, width=1024, n_mul=7400)
    return prog, wit, wc


def gf2_items(prog):
    """item counts of the GF(2) vectors this module can name exactly: one `in` item per Input, one `corr` item per Mul"""
    g = prog[prog["domain"] == 0]
    return {"in": int((g["opcode"] == 0).sum()), "corr": int((g["opcode"] == 6).sum())}


def item_op(prog, domain, vec, item):
    """index of the op that consumes item `item` of the vector `in` / `corr` of domain 0 (GF(2)) / 1 (Z64): the item's Input /
    Mul gate (None past the last one)"""
    opcode = 0 if vec == "in" else 6
    at = np.flatnonzero((prog["domain"] == domain) & (prog["opcode"] == opcode))
    return int(at[item]) if item < len(at) else None


def answer(oracle, prog, wc, proof: bytes, threads=4):
    """the oracle's (strict, compat) answers: each a bool, or ("err", code)"""
    out = []
    for strict in (True, False):
        try:
            out.append(oracle.verify(prog, wc, proof, threads=threads, strict=strict))
        except oracle.OracleError as e:
            out.append(("err", e.code))
    return tuple(out)


def answers(oracle, prog, wc, entries):
    """answer() of every (label, proof) entry, in order (the oracle runs beside itself: ctypes calls release the GIL)"""
    with ThreadPoolExecutor(max(1, min(4, (os.cpu_count() or 1) // 4))) as pool:
        return list(pool.map(lambda e: answer(oracle, prog, wc, e[1]), entries))


def classes(ans):
    """(accepted, refused, malformed) counts of strict answers"""
    strict = [a[0] for a in ans]
    return sum(a is True for a in strict), sum(a is False for a in strict), sum(isinstance(a, tuple) for a in strict)


_cache = {}


def case(oracle, seeds, name, targets=proof_mutate.ALL_TARGETS):
    """-> dict(prog, w2, w64, wc, good, entries [(label, bytes)], answers [(strict, compat)]), computed once per process"""
    key = (name, targets)
    if key not in _cache:
        prog, w2, w64, wc = circuit(name)
        good = oracle.prove(prog, w2, w64, wc, seeds)
        entries = list(proof_mutate.catalogue(good, targets=targets, gf2_items=gf2_items(prog)))
        _cache[key] = dict(prog=prog, w2=w2, w64=w64, wc=wc, good=good, entries=entries, answers=answers(oracle, prog, wc, entries))
    return _cache[key]
