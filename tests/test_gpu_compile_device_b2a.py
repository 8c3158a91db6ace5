"""The device compiler on programs with B2A ops (RV_COMPILE_DEVICE | RV_COMPILE_DEVICE_Z64 | RV_COMPILE_DEVICE_B2A,
csrc/compile_dev.hip): the host compiler's Compiled field by field for whole programs in both gate-stream forms and for a stream's
pieces, the host compiler's status on op-list errors, byte-identical proofs and equal answers, and the streams with every piece
compiled on the GPU.  Every case compares against the host path, rv_prove or the committed golden proofs, never against the device
path itself.

"taken" means (host status, path, diff) == (0, 1, 0) from the compare hooks.  In the plain form a whole program is taken exactly when
its K = 1 compile is the host compiler's final answer (k1_final); in the lazy-sum form (RV_COMPILE_WHOLE_PROVER) every valid program
is."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import circuits
from conftest import GOLDEN, golden_matches, golden_ops
from reverie_amd.ops import B2A, GF2, OP_DTYPE, SizeHint, Z64, program
from test_gpu_compile_device_z64 import (_compile_status, _edges, _no_times, _pieces, _tensor, compare, compare_chunk, device_chunks, gen_mixed,
                                         k1_final)

pytestmark = pytest.mark.gpu

WP, KEEP, DEV, DEVZ, B2A_BIT = 1, 2, 4, 12, 32
F = DEVZ | B2A_BIT
META = json.load(open(os.path.join(GOLDEN, "proofs.json")))
KW = {"device_compile": True, "device_z64": True, "device_b2a": True}


def _L():
    from reverie_amd import _lib

    return _lib.lib()


def check_both_forms(prog, wc, monkeypatch, what=""):
    """the plain form: taken exactly when the K = 1 compile is final; the lazy-sum form: taken; no difference either way"""
    final = k1_final(prog, wc, monkeypatch)
    rc, path, diff = compare(prog, wc, F)
    assert (rc, diff) == (0, 0) and path == int(final), (what, "plain", rc, path, diff, final)
    assert compare(prog, wc, F | WP) == (0, 1, 0), (what, "lazy")
    return final


def inputs(n, first=0):
    return [GF2.Input(first + i) for i in range(n)]


# ---- 1. one adder ----
def one_adder():
    return program(inputs(64) + [B2A(0, 0), Z64.AddConst(1, 0, 5)]), (2, 64)


def test_one_adder(monkeypatch):
    prog, wc = one_adder()
    assert not check_both_forms(prog, wc, monkeypatch)  # (about 190 levels of a few gates: the host compiler recompiles it with lazy sums)
    # without the new bit the program stays on the host, as before
    assert compare(prog, wc, DEVZ) == (0, 0, 0) and compare(prog, wc, DEVZ | WP) == (0, 0, 0)


# ---- 2. operand edges ----
def edge_programs():
    tail = [Z64.AddConst(1, 0, 5)]
    sums = inputs(8, 64)
    for k in range(64):  # sums of two rows (even k) and of three (odd k), read once: they stay lazy sums in the lazy-sum form
        sums.append(GF2.Add(k, 64 + k % 8, 64 + (k + 1) % 8))
        if k % 2:
            sums.append(GF2.Add(k, k, 64 + (k + 3) % 8))
    muls = inputs(2, 64) + [GF2.Mul(0, 64, 65)]
    for k in range(1, 64):  # wire k: a Mul gate at level k + 1 (every eighth one starts again at level 1)
        muls.append(GF2.Mul(k, 64, 65) if k % 8 == 0 else GF2.Mul(k, k - 1, 64 + k % 2))
    return {
        "never_written": ([B2A(0, 0)] + tail, (2, 64)),
        "constants": ([GF2.Const(i, (0xA53C >> (i % 16)) & 1) for i in range(64)] + [B2A(0, 0)] + tail, (2, 64)),
        "same_row": ([GF2.Input(0)] + [GF2.AddConst(i, 0, 0) for i in range(1, 64)] + [B2A(0, 0)] + tail, (2, 64)),
        "same_row_and_constants": ([GF2.Input(0)] + [GF2.AddConst(i, 0, i & 1) for i in range(1, 48)] + [B2A(0, 0)] + tail, (2, 64)),
        "lazy_sums": (sums + [B2A(0, 0)] + tail, (2, 72)),
        "mul_levels": (muls + [B2A(0, 0)] + tail, (2, 66)),
        "same_window_twice": (inputs(64) + [B2A(0, 0), B2A(1, 0), Z64.Add(2, 0, 1)], (3, 64)),
        "overlapping_windows": (inputs(96) + [B2A(0, 0), B2A(1, 32), Z64.Sub(2, 0, 1)], (3, 96)),
        "window_ends_at_the_last_wire": (inputs(100) + [B2A(0, 36)] + tail, (2, 100)),
        "result_overwritten": (inputs(64) + [B2A(0, 0), Z64.Const(0, 7), Z64.AddConst(1, 0, 1), B2A(1, 0)], (2, 64)),
        "result_never_read": (inputs(64) + [B2A(0, 0)], (1, 64)),
        "result_feeds_mul_and_assert": (inputs(64) + [B2A(0, 0), Z64.Input(1), Z64.Mul(2, 0, 1), Z64.AssertZero(2), Z64.AssertZero(0), Z64.Mul(0, 0, 0)], (3, 64)),
        "between_randoms": (inputs(64) + [GF2.Random(64), Z64.Random(1), Z64.Input(2), B2A(0, 0), GF2.Random(65), Z64.Random(3), GF2.Mul(66, 64, 65),
                                          Z64.Mul(4, 1, 3), B2A(5, 3), GF2.Random(0), Z64.Random(0), GF2.AssertZero(66), GF2.Input(1)], (6, 67)),
        "sources_rewritten_between": (inputs(64) + [B2A(0, 0)] + [GF2.Mul(i, i, (i + 1) % 64) for i in range(0, 64, 3)] + [B2A(1, 0), GF2.Input(5), B2A(2, 0)],
                                      (3, 64)),
    }


@pytest.mark.parametrize("name", sorted(edge_programs()))
def test_operand_edges(monkeypatch, name):
    ops, wc = edge_programs()[name]
    check_both_forms(program(ops), wc, monkeypatch, name)


def test_operand_edges_in_one_program(monkeypatch):
    """the edge programs one after the other over the same wires: every B2A then reads what the programs before it left"""
    ops, w64, w2 = [], 0, 0
    for name in sorted(edge_programs()):
        o, wc = edge_programs()[name]
        ops += o
        w64, w2 = max(w64, wc[0]), max(w2, wc[1])
    prog = program(ops)
    assert int((prog["domain"] == 2).sum()) >= 18
    check_both_forms(prog, (w64, w2), monkeypatch)


# ---- 3. errors keep the host's code ----
def test_errors_keep_the_host_code():
    reserved = program(inputs(64) + [B2A(0, 0), Z64.AddConst(0, 0, 1)])
    reserved["reserved"][64] = 1
    cases = {
        "source_window_past_the_wires": (program(inputs(64) + [B2A(0, 1)]), (1, 64), 3),
        "source_far_out": (program(inputs(64) + [B2A(0, 0xFFFFFFF0)]), (1, 64), 3),
        "dst_past_the_wires": (program(inputs(64) + [B2A(1, 0)]), (1, 64), 3),
        "reserved": (reserved, (1, 64), 5),
        "error_behind_a_b2a": (program(inputs(64) + [B2A(0, 0), GF2.Mul(64, 0, 1)]), (1, 64), 3),
    }
    for name, (prog, wc, want_rc) in cases.items():
        for flags in (F, F | WP):
            assert compare(prog, wc, flags) == (want_rc, 0, 0), (name, flags)
        rc, path, diff = compare_chunk(prog, wc, (3, 1, 7, 2, 8, 1), F)
        assert (rc, path, diff) == (want_rc, 0, 0), name
        want = _compile_status(prog, wc)
        assert want[0] == want_rc, name
        for wp in (False, True):
            got = _compile_status(prog, wc, whole_prover=wp, **KW)
            assert got[0] == want_rc and not got[2], name
    # what stays the host compiler's whatever the ops: KEEP_WIRES, a SizeHint that grows a wire count
    prog, wc = one_adder()
    assert compare(prog, wc, F | WP | KEEP) == (0, 0, 0)
    grown = program([SizeHint(2, 64)] + inputs(64) + [B2A(0, 0)])
    assert compare(grown, (1, 1), F | WP) == (0, 0, 0)
    assert compare(grown, (2, 64), F | WP) == (0, 1, 0)


# ---- 4. a wide program: final in the plain form ----
_WIDE = {}


def wide_program(n_b2a=128):
    if n_b2a not in _WIDE:
        ops = inputs(64 * n_b2a) + [B2A(j, 64 * j) for j in range(n_b2a)] + [Z64.Add(n_b2a, 0, 1)]
        _WIDE[n_b2a] = (program(ops), (n_b2a + 1, 64 * n_b2a))
    return _WIDE[n_b2a]


def test_wide_program_is_taken_in_both_forms(monkeypatch):
    n_b2a = 128
    while not k1_final(*wide_program(n_b2a), monkeypatch):  # (wider when the rule says otherwise)
        n_b2a *= 2
        assert n_b2a <= 1024
    prog, wc = wide_program(n_b2a)
    assert compare(prog, wc, F) == (0, 1, 0)
    assert compare(prog, wc, F | WP) == (0, 1, 0)


# ---- 5. random programs ----
def gen_b2a(rng, n_ops, w64, w2, z_share, valid=False, randoms=True):
    """gen_mixed's program with B2A ops at random places over random windows (w2 >= 64): about one in 60 ops.  valid: the witness still
    satisfies every AssertZero -- a B2A then writes a Z64 wire of its own behind gen_mixed's, which nothing reads but a Z64 op put
    right behind it.  -> (program, GF(2) witness, Z64 witness, wire counts)"""
    assert w2 >= 64
    prog, wit2, wit64 = gen_mixed(rng, n_ops, w64, w2, z_share, valid=valid, randoms=randoms)
    n_b2a = max(1, n_ops // 60)
    at = np.sort(rng.integers(0, len(prog) + 1, n_b2a))
    out, last = [], 0
    for j, a in enumerate(at):
        out.append(prog[last:a])
        last = a
        src = int(rng.integers(0, w2 - 63)) if rng.random() < 0.8 else w2 - 64
        if valid:
            dst = w64 + j % 3
            out.append(program([B2A(dst, src), Z64.MulConst(dst, dst, 3)]))
        else:
            dst = int(rng.integers(0, w64))
            out.append(program([B2A(dst, src)]))
    out.append(prog[last:])
    return np.concatenate(out), wit2, wit64, (w64 + (3 if valid else 0), w2)


SEEDS = list(range(40))


@pytest.mark.parametrize("group", range(8))
def test_random_programs(monkeypatch, group):
    for seed in SEEDS[5 * group:5 * group + 5]:
        rng = np.random.default_rng(0xB2A000 + seed)
        n_ops = int(rng.integers(200, 3001))
        w64 = int(rng.choice([3, 12, 65, 300]))
        w2 = int(rng.choice([64, 65, 70, 100, 257, 600]))
        prog, _, _, wc = gen_b2a(rng, n_ops, w64, w2, float(rng.choice([0.1, 0.5, 0.9])))
        assert bool((prog["domain"] == 2).any())
        check_both_forms(prog, wc, monkeypatch, seed)


# ---- 6. chunks ----
def chunk_pieces():
    written = inputs(10) + [GF2.Mul(3, 0, 1), GF2.Add(4, 2, 3), GF2.AddConst(5, 70, 1), GF2.Const(6, 1), GF2.Mul(63, 4, 64), GF2.Add(62, 62, 63)]
    return {
        "one_b2a_on_carried_rows": (program([B2A(0, 0)]), (1, 64)),
        "b2a_reads_the_piece_s_writes": (program(written + [B2A(0, 0), GF2.Mul(7, 7, 8), Z64.AddConst(1, 0, 3)]), (2, 80)),
        "two_b2a_and_z64_ops": (program([Z64.Input(3), B2A(0, 0), GF2.Mul(70, 0, 1), GF2.Input(33), B2A(1, 16), Z64.Mul(2, 0, 1), Z64.Add(3, 2, 3),
                                         Z64.AssertZero(1), Z64.Sub(0, 3, 4), GF2.AssertZero(70)]), (5, 80)),
        "empty": (np.zeros(0, OP_DTYPE), (3, 70)),
    }


@pytest.mark.parametrize("mask_phase", [0, 1, 66, 127])  # (66: the 190 masks of a B2A straddle a cipher-block boundary)
def test_chunks(mask_phase):
    for mask64_phase in (0, 1):
        start = (mask_phase, mask64_phase, 7, 2, 8, 1)  # (all four transcript offsets nonzero)
        for name, (prog, wc) in chunk_pieces().items():
            assert compare_chunk(prog, wc, start, F) == (0, 1, 0), (name, start)  # (diff 0: the write-back level included)
    # without the new bit a B2A piece stays on the host
    prog, wc = chunk_pieces()["one_b2a_on_carried_rows"]
    assert compare_chunk(prog, wc, (mask_phase, 0, 7, 2, 8, 1), DEVZ) == (0, 0, 0)


def test_random_chunks():
    rng = np.random.default_rng(0xB2AC)
    for k in range(6):
        prog, _, _, wc = gen_b2a(rng, int(rng.integers(100, 900)), 12, int(rng.choice([64, 100, 257])), 0.5)
        start = (int(rng.integers(0, 128)), int(rng.integers(0, 2)), int(rng.integers(1, 99)), int(rng.integers(1, 99)), int(rng.integers(1, 99)),
                 int(rng.integers(1, 99)))
        assert compare_chunk(prog, wc, start, F) == (0, 1, 0), (k, start)


# ---- 7. streams ----
_BRIDGED = []


def bridged_program():
    """the circuit of test_gpu_compile_device_z64.py::test_stream_b2a_piece_in_the_middle: a mixed program with a B2A bridge in the
    middle, cut so that the bridge is a piece of its own -> (program, GF(2) witness, Z64 witness, wire counts, cuts)"""
    if not _BRIDGED:
        rng = np.random.default_rng(0x2643)
        prog, w2, w64 = gen_mixed(rng, 2500, 12, 12, 0.5, valid=True, randoms=False)
        wc = (12, 12)
        half = len(prog) // 2
        bridge = program([GF2.Const(wc[1] + i, (0x5A >> (i % 8)) & 1) for i in range(64)] + [B2A(wc[0], wc[1]), Z64.AddConst(wc[0], wc[0], 1)])
        full = np.concatenate([prog[:half], bridge, prog[half:]])
        cuts = [half // 2, half, half + len(bridge), half + len(bridge) + (len(prog) - half) // 2]
        _BRIDGED.append((full, w2, w64, (wc[0] + 1, wc[1] + 64), cuts))
    return _BRIDGED[0]


def _stream(prog, w2, w64, wc, seeds, cuts, on_gpu):
    from reverie_amd.stream import StreamingProver

    sp = StreamingProver(wc, seeds=seeds, **KW)
    try:
        for part, a, b in _pieces(prog, w2, w64, cuts):
            sp.feed(_tensor(part) if on_gpu else part, a, b)
        comm = sp.commit()
        for part, a, b in _pieces(prog, w2, w64, cuts):
            sp.feed(_tensor(part) if on_gpu else part, a, b)
        proof = sp.finish()
    finally:
        sp.close()
    assert proof.comm == comm
    return proof


def _d2h():
    traffic = (C.c_uint64 * 2)()
    assert _L().rv_hook_stream_op_traffic(traffic) == 0
    return int(traffic[1])


@pytest.mark.parametrize("on_gpu", [False, True])
def test_stream_every_piece_on_the_device(rule_seeds, on_gpu):
    import reverie_amd

    full, w2, w64, wc, cuts = bridged_program()
    parts = [full[a:b] for a, b in _edges(full, cuts)]
    assert [bool((p["domain"] == 2).any()) for p in parts] == [False, False, True, False, False]
    want = bytes(reverie_amd.Proof.new(full, w2, w64, wc, seeds=rule_seeds))
    before, d2h = device_chunks(), _d2h()
    assert bytes(_stream(full, w2, w64, wc, rule_seeds, cuts, on_gpu)) == want
    assert device_chunks() - before == 5  # (pass 2 takes pass 1's compiled pieces from the cache)
    assert _d2h() - d2h == 0  # (a device feed copies no piece to the host; a host feed never did)


def test_stream_one_shot_calls(rule_seeds):
    import reverie_amd
    from reverie_amd.stream import evaluate_streaming, prove_streaming, prove_streaming_batch, verify_streaming

    full, w2, w64, wc, _ = bridged_program()
    CH = 1024
    n_pieces = -(-len(full) // CH)
    circ = reverie_amd.Circuit(full, wc)
    proof = reverie_amd.Proof.new(circ, w2, w64, seeds=rule_seeds)
    ev_host = evaluate_streaming(full, w2, w64, wc, max_chunk_ops=CH, values=True)
    seeds2 = np.stack([np.roll(np.asarray(rule_seeds, np.uint8).reshape(256, 16), b, axis=0) for b in range(2)])
    g2, z2 = np.tile(np.asarray(w2, np.uint8), (2, 1)), np.tile(np.asarray(w64, np.uint64), (2, 1))
    # (two witnesses of the batch: the same values under two seed sets, so two different proofs)
    wants = [bytes(p) for p in prove_streaming_batch(full, g2, z2, wc, seeds=seeds2, max_chunk_ops=CH)]
    for ops in (full, _tensor(full)):
        before, d2h = device_chunks(), _d2h()
        got, _ = prove_streaming(ops, w2, w64, wc, seeds=rule_seeds, max_chunk_ops=CH, **KW)
        assert bytes(got) == bytes(proof) and device_chunks() - before == n_pieces
        before = device_chunks()
        ok, _ = verify_streaming(ops, wc, proof, max_chunk_ops=CH, **KW)
        assert ok and device_chunks() - before == n_pieces
        before = device_chunks()
        ev = evaluate_streaming(ops, w2, w64, wc, max_chunk_ops=CH, values=True, **KW)
        assert device_chunks() - before == n_pieces
        assert bool(ev.ok[0]) and np.array_equal(ev.ok, ev_host.ok) and np.array_equal(ev.gf2, ev_host.gf2) and np.array_equal(ev.z64, ev_host.z64)
        before = device_chunks()
        proofs = prove_streaming_batch(ops, g2, z2, wc, seeds=seeds2, max_chunk_ops=CH, **KW)
        assert [bytes(p) for p in proofs] == wants and device_chunks() - before == n_pieces
        assert _d2h() - d2h == 0
    assert wants[0] == bytes(reverie_amd.Proof.new(circ, w2, w64, seeds=seeds2[0]))
    circ.close()


# ---- 8. end to end ----
def proof_programs():
    prog, wc = one_adder()
    bits = [(0x9E3779B97F4A7C15 >> i) & 1 for i in range(64)]
    out = [("one_adder", prog, bits, [], wc)]
    rng = np.random.default_rng(0xB2A8)
    prog, w2, w64, _ = circuits.random_mixed(rng, 300)
    assert bool((prog["domain"] == 2).any())
    out.append(("random_mixed", prog, w2, w64, (12, 90)))  # (its SizeHint(12, 90) grows nothing at these wire counts)
    prog, w2, w64, wc = gen_b2a(np.random.default_rng(0xB2A9), 900, 20, 80, 0.5, valid=True, randoms=False)
    out.append(("gen_b2a", prog, w2, w64, wc))
    prog, wc = wide_program()
    out.append(("wide", prog, [int(b) for b in np.random.default_rng(5).integers(0, 2, wc[1])], [], wc))
    return out


@pytest.mark.parametrize("k", range(4))
def test_proofs_and_info(rule_seeds, monkeypatch, k):
    import torch

    import reverie_amd

    name, prog, w2, w64, wc = proof_programs()[k]
    final = k1_final(prog, wc, monkeypatch)
    assert final == (name == "wide"), name
    t = torch.from_numpy(prog.view(np.uint8).reshape(len(prog), 24).copy()).cuda()
    want = None
    for wp in (False, True):
        host = reverie_amd.Circuit(prog, wc, whole_prover=wp)
        dev = reverie_amd.Circuit(prog, wc, whole_prover=wp, **KW)
        dten = reverie_amd.Circuit.from_device_ops(t, wc, whole_prover=wp, device_z64=True, device_b2a=True)
        on_device = wp or final
        assert not host.compiled_on_device and dev.compiled_on_device == on_device and dten.compiled_on_device == on_device, (name, wp)
        assert _no_times(dev.info) == _no_times(host.info) == _no_times(dten.info), (name, wp)
        assert host.info["b2a"] == int((prog["domain"] == 2).sum())
        ph = reverie_amd.Proof.new(host, w2, w64, seeds=rule_seeds)
        want = want or bytes(ph)
        assert bytes(ph) == want, (name, wp)
        for c in (dev, dten):
            p = reverie_amd.Proof.new(c, w2, w64, seeds=rule_seeds)
            assert bytes(p) == want, (name, wp)
            assert p.verify(host, strict=True) and ph.verify(c, strict=True), (name, wp)
        for c in (host, dev, dten):
            c.close()


def _grows(ops, wc):
    return any(o[0] == 3 and (o[4] > wc[0] or o[5] > wc[1]) for o in ops)


GOLDEN_B2A = [n for n, m in META.items() if any(o[0] == 2 for o in golden_ops(m)) and not _grows(golden_ops(m), tuple(m["wire_counts"]))]


def test_golden_cases_with_b2a_exist():
    assert "ref_test" in GOLDEN_B2A


@pytest.mark.parametrize("name", GOLDEN_B2A)
def test_golden_proofs(oracle, rule_seeds, name):
    import reverie_amd

    m = META[name]
    prog, wc = program(golden_ops(m)), tuple(m["wire_counts"])
    assert compare(prog, wc, F | WP) == (0, 1, 0)
    for wp in (True, False):
        c = reverie_amd.Circuit(prog, wc, whole_prover=wp, **KW)
        assert c.compiled_on_device or not wp
        proof = reverie_amd.Proof.new(c, m["wit_gf2"], [int(x) for x in m["wit_z64"]], seeds=rule_seeds)
        assert golden_matches(oracle, name, m, bytes(proof)), (name, wp)
        c.close()


# ---- 9. the context's flags ----
def test_prove_ops_under_context_flags(rule_seeds):
    import reverie_amd

    name, prog, w2, w64, wc = proof_programs()[3]
    assert len(prog) >= 1024  # (shorter programs bypass the ops cache)
    L = _L()
    plain, flagged = reverie_amd.Context(0), reverie_amd.Context(0)
    flagged.set_compile_flags(F)
    want = bytes(reverie_amd.Proof.new(prog, w2, w64, wc, seeds=rule_seeds, ctx=plain))
    # the last device compile of the process becomes a two-op program's; the cold rv_prove_ops then leaves the adders' rounds there
    tiny = program([GF2.Input(0), GF2.Mul(1, 0, 0)])
    assert compare(tiny, (0, 2), DEV) == (0, 1, 0)
    laps = (C.c_double * 6)()
    assert L.rv_hook_compile_device_laps(laps) == 0 and laps[5] < 8
    for _ in range(2):  # cold, then from the ops cache
        got = reverie_amd.Proof.new(prog, w2, w64, wc, seeds=rule_seeds, ctx=flagged)
        assert bytes(got) == want
        assert got.verify(prog, wc, ctx=flagged, strict=True)
    assert L.rv_hook_compile_device_laps(laps) == 0 and laps[5] >= 64  # (an adder's carry chain is 62 Mul gates deep)
    with pytest.raises(reverie_amd.ReverieError):
        flagged.set_compile_flags(DEV | B2A_BIT)
    flagged.set_compile_flags(0)
    assert bytes(reverie_amd.Proof.new(prog, w2, w64, wc, seeds=rule_seeds, ctx=flagged)) == want
    plain.close()
    flagged.close()
