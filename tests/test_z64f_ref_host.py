"""tests/z64f_ref.py against the CPU oracle, through production's own records and without a device: the proof that the reference of
one fused Z64 level (what tests/test_gpu_z64_fused_level.py compares k_z64_fused with) computes the protocol.

Prover: the records rv_hook_z64_fused_gates returns for eligible programs are run level by level at first_block = 0 for all 256
repetitions under the rule seeds; every repetition's preprocessing and online stream must hash (tests/b3_ref.py) to the oracle's
commitment streams 2 and 3.  Verifier: the values a proof would carry are taken from the prover reference's own streams under the
oracle's challenge; the verifier reference must reproduce the prover's online words in every opened repetition and its preprocessing
words in every other one.  Last, the record counts and level tables of the hand-made cases the GPU file runs are pinned here."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import b3_ref
import class_mix64 as cm
import z64f_cases as zc
import z64f_ref as zr
from conftest import GOLDEN
from reverie_amd.ops import OP_ASSERTZERO, Z64, program

META = json.load(open(os.path.join(GOLDEN, "proofs.json")))


def _z64_mix():
    m = META["z64_mix"]
    return program([tuple(o) for o in m["ops"]]), [int(x) for x in m["wit_z64"]], tuple(m["wire_counts"])


def _z64_mix_eligible():
    """the golden circuit without its Random gate and the three gates behind it, and with a sixth Input (five leave the first Mul's mask
    pair astride two cipher blocks): what of z64_mix the fused path can take"""
    prog, wit, wc = _z64_mix()
    drop = np.isin(prog["dst"], (12, 13, 14)) & (prog["opcode"] != OP_ASSERTZERO) | (prog["opcode"] == OP_ASSERTZERO) & (prog["a"] == 14)
    assert drop.sum() == 4
    kept = prog[~drop]
    return np.concatenate([kept[:5], program([Z64.Input(17)]), kept[5:]]), wit + [9], wc


PROGRAMS = {
    "mixed": lambda: cm.class_mix64(cm.MIXED, cm.SEED),
    "rotation-edges": lambda: cm.class_mix64(cm.ROTATION, cm.SEED, values="edges"),
    "interleaved": lambda: cm.class_mix64(cm.INTERLEAVED, cm.SEED, order="interleaved"),
    "runs8": lambda: cm.class_mix64(cm.runs_spec(8), cm.SEED, inputs=("runs", 8)),
    "z64_mix-eligible": _z64_mix_eligible,
}


def _stream_digests(st):
    as_bytes = lambda a: np.ascontiguousarray(a.astype("<u8")).view(np.uint8).reshape(len(a), -1)  # noqa: E731
    return b3_ref.hash_bytes(as_bytes(st.pre)), b3_ref.hash_bytes(as_bytes(st.on))


@pytest.mark.parametrize("name", sorted(PROGRAMS))
def test_reference_hashes_to_the_oracles_commitment_and_verifier_agrees(oracle, rule_seeds, name):
    prog, wit, wc = PROGRAMS[name]()
    case = zc.from_program(name, prog, wit, wc)
    assert case.on_words and case.pre_words and len(case.wit) == case.n_in
    pr = zc.run_ref(case, rule_seeds, None, 0)
    assert pr.err == 0 and not (pr.on == zr.FILL).all(1).any()
    h, streams, comm = oracle.commit(prog, [], wit, wc, rule_seeds)
    pre, on = _stream_digests(pr)
    assert (pre == streams[:, 2]).all(), np.flatnonzero((pre != streams[:, 2]).any(1))[:8]
    assert (on == streams[:, 3]).all(), np.flatnonzero((on != streams[:, 3]).any(1))[:8]
    # the verifier, on what an honest proof carries under the oracle's challenge
    omit = oracle.challenge(comm)
    opened = omit < 8
    assert 0 < opened.sum() < 256
    vr = zc.run_ref(case, rule_seeds, omit, 0, sup=zc.honest_sup(case, pr, omit))
    assert (vr.on[opened] == pr.on[opened]).all() and (vr.pre[~opened] == pr.pre[~opened]).all()
    assert (vr.pre[opened] == pr.pre[opened]).all()  # (the supplied corrections, stored as they came)
    assert vr.err == 0
    # the public corrections of an opened repetition are value - reconstruct(mask) of the prover's run
    # (of the SSA ids one gate alone writes, and that gate a linear one or a Const: mask row, value and correction then belong together)
    written = np.bincount(case.gates["dst"][case.gates["op"] != zr.ASSERT], minlength=case.n_ssa)
    for g in case.gates:
        ssa = int(g["dst"])
        if zc.CLASS[int(g["op"])] == 1 or g["op"] == zr.CONST:
            if written[ssa] != 1:
                continue
            assert (vr.wcorr[ssa, opened] == (pr.v[ssa] - pr.wmask[ssa].sum(1))[opened]).all(), ssa


def test_a_failing_assert_zero_shows_in_opened_repetitions_only(oracle, rule_seeds):
    good, bad = zc.operands(False), zc.operands(True)
    seeds = rule_seeds[:32]
    for case, code in ((good, 0), (bad, zr.E_WITNESS_INVALID)):
        pr = zc.run_ref(case, seeds, None, 0)
        assert pr.err == code
        none, mix = zc.omits(32, "none"), zc.omits(32, "mix")
        assert zc.run_ref(case, seeds, none, 0, sup=zc.honest_sup(case, pr, none)).err == 0
        assert zc.run_ref(case, seeds, mix, 0, sup=zc.honest_sup(case, pr, mix)).err == (zr.DEV_ZERO_CHECK if code else 0)
        # ... and a launch that leaves quad word 0 out cannot see the prover's clear values
    pr = zc.run_ref(bad, rule_seeds[:96], None, 0, qg0=1, qgn=2)
    assert pr.err == 0 and (pr.v == zr.FILL).all() and (pr.on[:32] == zr.FILL).all() and not (pr.on[32:] == zr.FILL).all(1).any()


def test_z64_mix_itself_is_not_eligible():
    prog, wit, wc = _z64_mix()
    gates, levels, runs, why, sizes = zc.fused_gates(prog, wc)
    assert why == cm.WHY_GATE and len(gates) == 0 and len(levels) == 0  # (a Random gate: no table)


def test_gates_hook_agrees_with_the_levels_hook_and_fills_by_count():
    from reverie_amd import _lib

    lib = _lib.lib()
    prog, wit, wc = cm.class_mix64(cm.MIXED, cm.SEED)
    gates, levels, runs, why, sizes = zc.fused_gates(prog, wc)
    want, why2 = cm.fused_levels(prog, wc)
    assert why == why2 == 0 and [(int(l[1] - l[0]), int(l[2] - l[1]), int(l[3] - l[2])) for l in levels] == want
    assert len(gates) == int(levels[-1, 3]) and runs.tolist() == [[0, 17]]  # 34 Inputs
    z = prog[prog["domain"] == 1]
    assert sizes[1] == 34 + 2 * int((gates["op"] == zr.MUL).sum()) and sizes[4] == 34 and len(gates) == len(z)
    for lv in levels:  # Mul | linear | other inside every level
        cls = [zc.CLASS[int(op)] for op in gates["op"][lv[0]:lv[3]]]
        assert cls == sorted(cls) and cls.count(0) == lv[1] - lv[0] and cls.count(1) == lv[2] - lv[1]
    # a short buffer takes the first entries and nothing behind them; the counts stay whole
    head = (prog.ctypes.data_as(C.c_void_p), C.c_size_t(len(prog)), C.c_size_t(wc[0]), C.c_size_t(wc[1]), C.c_uint32(0))
    ng, nl, nr, e = C.c_size_t(0), C.c_size_t(0), C.c_size_t(0), C.c_int(-1)
    g2 = np.full(3 * 64, 0x77, np.uint8).view(zr.GATE)
    l2 = np.full((3, 4), 7, np.uint32)
    p = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    assert lib.rv_hook_z64_fused_gates(*head, p(g2), 2, C.byref(ng), p(l2), 2, C.byref(nl), None, 0, C.byref(nr), C.byref(e), None) == 0
    assert (ng.value, nl.value, nr.value, e.value) == (len(gates), len(levels), 1, 0)
    assert g2[:2].tobytes() == gates[:2].tobytes() and g2[2:].tobytes() == b"\x77" * 64 and (l2[:2] == levels[:2]).all() and (l2[2] == 7).all()
    assert lib.rv_hook_z64_fused_gates(*head, None, 2, C.byref(ng), None, 0, C.byref(nl), None, 0, C.byref(nr), C.byref(e), None) == 9  # RV_E_ARG
    assert lib.rv_hook_z64_fused_gates(*head, None, 0, None, None, 0, C.byref(nl), None, 0, C.byref(nr), C.byref(e), None) == 9
    assert lib.rv_hook_z64_fused_run(None, None) == 9


def test_stored_layout_map():
    for NQ, QW in ((8, 8), (24, 8), (16, 16), (64, 16)):
        P = zr.stored_index(NQ)
        assert sorted(P.tolist()) == list(range(NQ * 32)) and zr.qw_of(NQ) == QW
        for qg, ql, i in ((0, 0, 0), (0, 1, 0), (0, 0, 1), (NQ // QW - 1, QW - 1, 15), (NQ // QW - 1, 3, 7)):
            for j in (0, 1):
                assert P[(qg * QW + ql) * 32 + 2 * i + j] == qg * 32 * QW + i * 2 * QW + ql * 2 + j
        blocks = P.reshape(NQ // QW, QW * 32)  # rows of different groups never meet
        assert all(b.min() == k * QW * 32 and b.max() == (k + 1) * QW * 32 - 1 for k, b in enumerate(blocks))
    assert zr.qw_of(4) == 0 and zr.qw_of(12) == 0


def test_hand_made_cases_are_what_the_gpu_file_says():
    """record counts and level tables of every case of tests/test_gpu_z64_fused_level.py (each builder also asserts its own shape, and
    Case() that the records of a level are independent)"""
    assert zc.counters(9).counts() == [(0, 0, 3), (9, 2, 0)] and zc.counters(4).last_block() == 4 and zc.counters(12).last_block() == 12
    g = zc.counters(9).gates
    assert g["m"][g["op"] == zr.INPUT].tolist() == [1, 2, 3] and g["m"][g["op"] == zr.MUL].tolist() == [0, 4, 6, 8, 10, 12, 14, 16, 18]
    for jw in (4, 8):
        c = zc.shapes(jw)
        assert [x[0] for x in c.counts()][2:] == [1, jw - 1, jw, jw + 1, 8 * jw - 1, 8 * jw + 1, 100] and len(c.gates) < 400
        # several chunks per quad group on a whole chip, at every quad-group count of the GPU file
        assert all(cm.fused_grid(64 // jw, n_qg, 256, 100, 0, 0)[0] >= 2 for n_qg in (1, 2, 3, 4))
    for pad in (0, 1):
        for tail in (0, 1):
            for lay in ("run", "gap"):
                c = zc.placement(pad, tail, lay)
                mul = c.gates[c.gates["op"] == zr.MUL]
                assert c.on_words == pad + 4 + 80 + 16 + tail and (mul["eo"] % 2 == (4 + pad) % 2).all()
                ep = mul["ep"].astype(np.int64)
                assert (np.diff(ep[:4]) == 1).all() and ((np.diff(ep) == 1).all() if lay == "run" else np.diff(ep)[5] == 4)
    # both on_words parities and both eo parities occur
    assert {(zc.placement(p, t, "run").on_words % 2, p) for p in (0, 1) for t in (0, 1)} == {(0, 0), (1, 0), (0, 1), (1, 1)}
    for bad in (False, True):
        c = zc.operands(bad)
        g = c.gates
        mul = g[g["op"] == zr.MUL]
        assert {bool(a & zr.MASK_ROW) for a in mul["am"]} == {True, False} and {bool(a & zr.MASK_ROW) for a in mul["bm"]} == {True, False}
        assert (mul["a"] == mul["b"]).any() and ((g["op"] == zr.MULC) & (g["imm"] == 0)).any()
        assert set(zc.EDGE_VALUES) <= {int(x) for x in c.wit} and set(zc.EDGE_VALUES) <= {int(x) for x in g["imm"][g["op"] == zr.CONST]}
        assert int((g["op"] == zr.ASSERT).sum()) == 9 + bad
    for R in (32, 96, 64, 128, 256):
        o = zc.omits(R, "mix")
        per = 4 * zr.qw_of(R // 4)
        assert (o[4:8] < 8).all() and all(o[e - 1] < 8 and o[e] < 8 for e in range(per, R, per)) and (zc.omits(R, "none") == 8).all()
