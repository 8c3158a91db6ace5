"""Cleartext evaluation on the GPU at its edges, every output against the independent batched reference (tests/eval_ref.py):
schedule (a) with Z64 gates, the walking schedule's slice shapes and thread counts, batches split into parts (RV_EVAL_PART), the
compile modes, the output layouts of the C ABI, witness shapes and degenerate circuits.  Every case checks which schedule ran
(rv_hook_eval_schedules) and runs once more on a poisoned device block (RV_EVAL_POISON=1) with identical results."""
import ctypes as C
import hashlib

import numpy as np
import pytest

import bristol_gen
import circuits
import eval_ref
import z64_batch_circuits as zb
from reverie_amd.ops import B2A, GF2, OP_DTYPE, Z64, SizeHint, program
from test_gpu_eval import _bits_msb, _bytes_msb, _pad, _wide, random_program, schedules

pytestmark = pytest.mark.gpu

PER_LEVEL, WALK = 0, 1


@pytest.fixture(scope="module")
def rv():
    import reverie_amd

    reverie_amd.Context.default()
    return reverie_amd


def _wits(B, w2=None, w64=None):
    return (np.zeros((B, 0), np.uint8) if w2 is None else w2), (np.zeros((B, 0), np.uint64) if w64 is None else w64)


def same_as_ref(r, ref, gf2_cols=None):
    g, z, nf, ff = ref
    assert np.array_equal(r.n_failed, nf), np.nonzero(r.n_failed != nf)[0][:8]
    assert np.array_equal(r.ok, nf == 0)
    assert np.array_equal(r.first_failed_op, ff), np.nonzero(r.first_failed_op != ff)[0][:8]
    assert np.array_equal(r.gf2 if gf2_cols is None else r.gf2[:, gf2_cols], g)
    assert np.array_equal(r.z64, z)


def same(r1, r2):
    for f in ("ok", "n_failed", "first_failed_op", "gf2", "z64"):
        assert np.array_equal(getattr(r1, f), getattr(r2, f)), f


def run(c, w2, w64, ref, sched, monkeypatch, parts=1, gf2_cols=None):
    """evaluate_batch with values: equal to the reference, on schedule `sched` in `parts` parts; then once more on a poisoned device
    block, with identical results"""
    out = None
    for poison in ("0", "1"):
        monkeypatch.setenv("RV_EVAL_POISON", poison)
        s0 = schedules()
        r = c.evaluate_batch(w2, w64, values=True)
        s1 = schedules()
        assert (s1[0] - s0[0], s1[1] - s0[1]) == ((parts, 0) if sched == PER_LEVEL else (0, parts)), poison
        same_as_ref(r, ref, gf2_cols)
        if out is not None:
            same(r, out)
        out = r
    monkeypatch.delenv("RV_EVAL_POISON")
    return out


def per_level(info, S=1):
    """(GF(2) + 32 x Z64 items) per level and witness word, estimated from the compile info (eval_walks / the walking kernel's
    thread count use the exact gate counts)"""
    g2 = info["gf2_inputs"] + info["gf2_muls"] + info["gf2_linear"] + info["gf2_asserts"]
    g64 = info["z64_inputs"] + info["z64_muls"] + info["z64_linear"] + info["z64_asserts"] + info["b2a"]
    return (g2 + 32 * g64) / max(info["levels"], 1) * S


# ---------------------------------------------------------------- circuits
def wide_mixed(seed=1, layers=8, w2=16384, w64=2048, n_b2a=16, n_ctrl=8, asserts=2):
    """Wide levels of GF(2) AND / XOR and Z64 Mul / Add side by side (schedule (a)), B2A bridges from GF(2) layer 2 into the Z64
    layers after it, and AssertZero ops of both domains in the middle of the layers.  Assertion t checks ctrl_t * (a gate of the
    layer): the last n_ctrl GF(2) and Z64 Inputs are control columns, so that a witness fails exactly the assertions whose control
    it sets (and whose gate is not zero).  -> (program, wire counts, GF(2) inputs, Z64 inputs)"""
    rng = np.random.default_rng(seed)
    n_in2, n_in64 = 256 + n_ctrl, 64 + n_ctrl
    ops = [GF2.Input(i) for i in range(n_in2)] + [Z64.Input(i) for i in range(n_in64)]
    p2, n2p, p64 = 0, n_in2 - n_ctrl, list(range(n_in64 - n_ctrl))
    nxt2, nxt64, t = n_in2, n_in64, 0
    for layer in range(layers):
        lay = []
        a, b, k = rng.integers(0, n2p, w2), rng.integers(0, n2p, w2), rng.random(w2) < 0.5
        lay += [GF2.Mul(nxt2 + g, p2 + a[g], p2 + b[g]) if k[g] else GF2.Add(nxt2 + g, p2 + a[g], p2 + b[g]) for g in range(w2)]
        a, b, k = rng.integers(0, len(p64), w64), rng.integers(0, len(p64), w64), rng.random(w64) < 0.5
        lay += [Z64.Mul(nxt64 + g, p64[a[g]], p64[b[g]]) if k[g] else Z64.Add(nxt64 + g, p64[a[g]], p64[b[g]]) for g in range(w64)]
        ops += lay[:w2 // 2] + lay[w2 + w64 // 2:]  # (the second halves of both: the assertions land between the halves)
        extra = []
        for _ in range(asserts):
            c = n_in2 - n_ctrl + t % n_ctrl
            extra += [GF2.Mul(nxt2 + w2, c, nxt2 + int(rng.integers(0, w2 // 2))), GF2.AssertZero(nxt2 + w2)]
            c = n_in64 - n_ctrl + t % n_ctrl
            extra += [Z64.Mul(nxt64 + w64, c, nxt64 + w64 // 2 + int(rng.integers(0, w64 // 2))), Z64.AssertZero(nxt64 + w64)]
            t += 1
        ops += extra + lay[w2 // 2:w2] + lay[w2:w2 + w64 // 2]
        p2, n2p, p64 = nxt2, w2, list(range(nxt64, nxt64 + w64))
        nxt2, nxt64 = nxt2 + w2 + 1, nxt64 + w64 + 1
        if layer == 2:
            for i in range(n_b2a):
                ops.append(B2A(nxt64, p2 + 64 * i))
                p64.append(nxt64)
                nxt64 += 1
    return program(ops), (nxt64, nxt2), n_in2, n_in64


def control_witness(rng, B, n_in2, n_in64, ctrl2, ctrl64, fail_at=()):
    """random witnesses with every control column zero but those of `fail_at`: {witness: [control k, ...]}; k sets GF(2) control
    k % len(ctrl2) and Z64 control k % len(ctrl64)"""
    w2 = rng.integers(0, 2, (B, n_in2)).astype(np.uint8)
    w64 = rng.integers(0, 1 << 64, (B, n_in64), dtype=np.uint64)
    w2[:, ctrl2] = 0
    w64[:, ctrl64] = 0
    for b, ks in dict(fail_at).items():
        for k in ks:
            w2[b, ctrl2[k % len(ctrl2)]] = 1
            w64[b, ctrl64[k % len(ctrl64)]] = int(rng.integers(1, 1 << 63))
    return w2, w64


def wide_witness(rng, B, n_in2, n_in64, fail_at=(), n_ctrl=8):
    return control_witness(rng, B, n_in2, n_in64, list(range(n_in2 - n_ctrl, n_in2)), list(range(n_in64 - n_ctrl, n_in64)), fail_at)


def mixed_deep(seed=7, n_asserts=12):
    """random_program (deep and narrow, B2A bridges, wires never written) without its own assertions, with 8 GF(2) and 4 Z64 control
    Inputs up front (witness columns 0-7 and 0-3; the program's own Inputs follow) and n_asserts AssertZero ops of both domains on
    ctrl * (a wire) spread through it.  -> (program, wire counts, GF(2) inputs, Z64 inputs, GF(2) controls, Z64 controls)"""
    rng = np.random.default_rng(seed)
    base, (n64, n2) = random_program(rng, n_gates=400, mixed=True, p_assert=0.0)
    ops = [tuple(o) for o in base.tolist()]
    head = [ops[0]] + [GF2.Input(90 + k) for k in range(8)] + [Z64.Input(n64 + k) for k in range(4)]
    body = ops[1:]
    at = sorted(rng.choice(np.arange(20, len(body)), n_asserts, replace=False).tolist(), reverse=True)
    for t, p in enumerate(at):
        w = int(rng.integers(0, 30))
        if t % 2:
            ins = [GF2.Mul(98, 90 + t % 8, w), GF2.AssertZero(98)]
        else:
            ins = [Z64.Mul(n64 + 4, n64 + t % 4, w % n64), Z64.AssertZero(n64 + 4)]
        body[p:p] = ins
    return program(head + body), (n64 + 5, n2), 18, 8, list(range(8)), list(range(4))


def deep_witness(rng, B, fail_p=0.3, fail_at=None):
    fail_at = fail_at if fail_at is not None else {b: rng.integers(0, 8, 2).tolist() for b in range(B) if rng.random() < fail_p}
    return control_witness(rng, B, 18, 8, list(range(8)), list(range(4)), fail_at)


# ---------------------------------------------------------------- 1. schedule (a) with Z64
@pytest.mark.parametrize("B", [1, 33, 100])
def test_schedule_a_with_z64(rv, monkeypatch, B):
    rng = np.random.default_rng(100 + B)
    # pure Z64: witness 0 satisfies the tail's assertions, the others fail them
    prog, wit, wc, _ = circuits.layered_z64(n_in=256, width=2048, n_mul=8000, fold_to=16)
    c = rv.Circuit(prog, wc, keep_wires=True)
    assert per_level(c.info) > 4 * 2048
    w64 = rng.integers(0, 1 << 64, (B, 256), dtype=np.uint64)
    w64[0] = wit
    ref = eval_ref.evaluate_layers(prog, wc, None, w64)
    assert ref[2][0] == 0 and (ref[2][1:] > 0).all()
    run(c, *_wits(B, None, w64), ref, PER_LEVEL, monkeypatch)
    # mixed: failures of both domains in the middle of levels, a different first one per witness
    prog, wc, n_in2, n_in64 = wide_mixed()
    c = rv.Circuit(prog, wc, keep_wires=True)
    assert per_level(c.info) > 2048 and c.info["b2a"] == 16
    fail_at = {b: sorted(set(rng.integers(0, 8, 1 + b % 3).tolist())) for b in range(B) if b % 3}
    w2, w64 = wide_witness(rng, B, n_in2, n_in64, fail_at)
    ref = eval_ref.evaluate(prog, wc, w2, w64)
    assert (ref[2][[b for b in range(B) if b not in fail_at]] == 0).all()
    if B > 1:
        assert (ref[2][list(fail_at)] > 0).all() and len(set(ref[3][list(fail_at)].tolist())) > 2
    run(c, w2, w64, ref, PER_LEVEL, monkeypatch)


# ---------------------------------------------------------------- 2. schedule (b): slices of one and more words
SLICE_B = [8192, 8193, 8224, 16465]  # W = 256 (S = 1), 257 (S = 2, last slice one word of one witness), 257 full, 515 (S = 3, 17)


@pytest.mark.parametrize("B", SLICE_B)
def test_walk_slices(rv, monkeypatch, B):
    rng = np.random.default_rng(B)
    # mixed, deep and narrow, with B2A (under 256 threads at S = 1)
    prog, wc = mixed_deep()[:2]
    c = rv.Circuit(prog, wc, keep_wires=True)
    assert per_level(c.info) < 2048
    w2, w64 = deep_witness(rng, B)
    ref = eval_ref.evaluate(prog, wc, w2, w64)
    assert 0 < (ref[2] > 0).sum() < B
    run(c, w2, w64, ref, WALK, monkeypatch)
    # pure Z64 chains, 16 lanes: 512 items per level, 1024 threads at every S
    prog, wit, wc = zb.chain_z64(lanes=16, rounds=32)
    c = rv.Circuit(prog, wc, keep_wires=True)
    assert 300 < per_level(c.info) < 2048
    w64 = rng.integers(0, 1 << 64, (B, 16), dtype=np.uint64)
    w64[::7] = wit
    ref = eval_ref.evaluate(prog, wc, None, w64)
    run(c, *_wits(B, None, w64), ref, WALK, monkeypatch)


@pytest.mark.parametrize("B", [8193, 16465])
def test_walk_slices_sha256(rv, monkeypatch, B):
    """SHA-256 (256 threads: per_level * S under 256), the digest of every witness against hashlib and 4 096 sampled wires plus the
    digest wires against the reference (the whole [B][1.2 * 10^5] vector is gigabytes)"""
    from reverie_amd import bristol

    text = bristol_gen.sha256_block()
    prog, info = bristol.parse(text)
    wc = info["wire_counts"]
    c = rv.Circuit(prog, wc, keep_wires=True)
    assert per_level(c.info, S=3) < 200
    rng = np.random.default_rng(B)
    msgs = [bytes(rng.integers(0, 256, int(rng.integers(0, 56)), dtype=np.uint8)) for _ in range(B)]
    w2 = np.array([_bits_msb(_pad(m)) for m in msgs], np.uint8)
    w2[w2 == 1] = rng.choice(np.array([1, 2, 0x80, 0xFF], np.uint8), int((w2 == 1).sum()))  # (any non-zero byte is a 1)
    outs = np.arange(info["n_wires"] - 256, info["n_wires"])
    cols = np.unique(np.concatenate([rng.choice(wc[1], 4096, replace=False), outs]))
    r = run(c, w2, None, eval_ref.evaluate(prog, wc, w2, gf2_cols=cols), WALK, monkeypatch, gf2_cols=cols)
    for k in range(B):
        assert _bytes_msb(r.gf2[k, outs]) == hashlib.sha256(msgs[k]).digest(), k


# ---------------------------------------------------------------- 3. parts
def _planted(B, part):
    """witness -> controls: failures in the first and last part and on both sides of every part boundary, different ones per part"""
    at = {0: [0], 1: [5], B - 1: [7], B - 2: [2, 6]}
    for p0 in range(part, B, part):
        at[p0 - 1] = [(p0 // part) % 8]
        at[p0] = [(p0 // part + 3) % 8]
    return at


@pytest.mark.parametrize("part", [32, 64, 96])
def test_parts_b1000(rv, monkeypatch, part):
    B = 1000
    rng = np.random.default_rng(part)
    n_parts = -(-B // (-(-part // 32) * 32))
    prog, wc, n_in2, n_in64 = wide_mixed()
    cases = [(rv.Circuit(prog, wc, keep_wires=True), prog, wc, *wide_witness(rng, B, n_in2, n_in64, _planted(B, part)), PER_LEVEL)]
    prog, wc = mixed_deep(11)[:2]
    cases.append((rv.Circuit(prog, wc, keep_wires=True), prog, wc, *deep_witness(rng, B, fail_at=_planted(B, part)), WALK))
    for c, prog, wc, w2, w64, sched in cases:
        ref = eval_ref.evaluate(prog, wc, w2, w64)
        whole = run(c, w2, w64, ref, sched, monkeypatch)
        monkeypatch.setenv("RV_EVAL_PART", str(part))
        same(run(c, w2, w64, ref, sched, monkeypatch, parts=n_parts), whole)
        monkeypatch.delenv("RV_EVAL_PART")
        assert len(set(ref[3][ref[3] >= 0].tolist())) > 3


def test_parts_b8193(rv, monkeypatch):
    B, part = 8193, 64
    rng = np.random.default_rng(8193)
    # schedule (a): the wide GF(2) circuit; every witness valid but the planted ones (one input bit flipped: different tail
    # assertions fail)
    prog, wc = _wide()
    _p, wit, _wc, _s = circuits.layered_gf2(n_in=512, width=16384, layers=3, seed=3)
    w2 = np.tile(np.asarray(wit, np.uint8), (B, 1))
    for i, b in enumerate(sorted({0, 1, B - 1, B - 2} | {p0 + d for p0 in range(part, B, 8 * part) for d in (-1, 0)})):
        w2[b, (37 * i) % 512] ^= 1
    ref = eval_ref.evaluate_layers(prog, wc, w2)
    assert 0 < (ref[2] > 0).sum() < B and len(set(ref[3][ref[3] >= 0].tolist())) > 3
    c = rv.Circuit(prog, wc, keep_wires=True)
    whole = run(c, w2, None, ref, PER_LEVEL, monkeypatch)
    monkeypatch.setenv("RV_EVAL_PART", str(part))
    same(run(c, w2, None, ref, PER_LEVEL, monkeypatch, parts=-(-B // part)), whole)
    # schedule (b): a deep mixed program
    monkeypatch.delenv("RV_EVAL_PART")
    prog, wc = mixed_deep(12)[:2]
    w2, w64 = deep_witness(rng, B, fail_at=_planted(B, 8 * part))
    ref = eval_ref.evaluate(prog, wc, w2, w64)
    c = rv.Circuit(prog, wc, keep_wires=True)
    whole = run(c, w2, w64, ref, WALK, monkeypatch)
    monkeypatch.setenv("RV_EVAL_PART", str(part))
    same(run(c, w2, w64, ref, WALK, monkeypatch, parts=-(-B // part)), whole)


# ---------------------------------------------------------------- 4. compile modes
def _compile_mode_programs():
    from test_eval_host import _random_gf2

    out = []
    prog, wc = _random_gf2(np.random.default_rng(5), 6000, n_wires=3000, n_z64=200)
    out.append(("random", prog, wc, True))
    prog, _w, wc, _s = circuits.layered_gf2(n_in=256, width=1024, layers=6, fold_to=16, seed=9)
    out.append(("layered", prog, wc, True))
    prog, wc = mixed_deep(13)[:2]
    out.append(("b2a", prog, wc, False))  # (the parallel compiler refuses B2A)
    return out


def test_compile_modes(rv, monkeypatch, capfd):
    B = 65
    rng = np.random.default_rng(65)
    for name, prog, wc, par in _compile_mode_programs():
        n2 = int(((prog["domain"] == 0) & (prog["opcode"] == 0)).sum())
        n64 = int(((prog["domain"] == 1) & (prog["opcode"] == 0)).sum())
        w2 = rng.integers(0, 2, (B, n2)).astype(np.uint8)
        w64 = rng.integers(0, 1 << 64, (B, n64), dtype=np.uint64)
        ref = eval_ref.evaluate(prog, wc, w2, w64)
        assert len(prog) >= 5000 or not par
        results = []
        for mode in ("default", "whole_prover", "parallel", "sequential"):
            if mode == "parallel" and not par:
                continue
            monkeypatch.setenv("RV_COMPILE_STATS", "1")
            if mode == "parallel":
                monkeypatch.setenv("RV_COMPILE_PAR_MIN", "1000")
                monkeypatch.setenv("RV_COMPILE_THREADS", "4")
            if mode == "sequential":
                monkeypatch.setenv("RV_COMPILE_SEQ", "1")
            capfd.readouterr()
            c = rv.Circuit(prog, wc, whole_prover=mode == "whole_prover", keep_wires=True)
            err = capfd.readouterr().err
            for k in ("RV_COMPILE_STATS", "RV_COMPILE_PAR_MIN", "RV_COMPILE_THREADS", "RV_COMPILE_SEQ"):
                monkeypatch.delenv(k, raising=False)
            assert ("parallel compiler (4 threads) returned 0" in err) == (mode == "parallel"), (name, mode, err)
            s0 = schedules()
            r = c.evaluate_batch(w2, w64, values=True)
            s1 = schedules()
            sched = PER_LEVEL if s1[0] > s0[0] else WALK
            same_as_ref(r, ref)
            results.append(run(c, w2, w64, ref, sched, monkeypatch))
        assert len(results) == (4 if par else 3)


# ---------------------------------------------------------------- 5. output layouts, witness shapes, degenerate circuits
def _raw(c, w2, w64, gf2=True, z64=True):
    """rv_evaluate_batch through ctypes with the value arrays the caller asks for (poisoned buffers where none is asked for)"""
    from reverie_amd import _lib

    B = w2.shape[0]
    st = np.zeros((B, 2), np.uint64)
    gv = np.full((B, c.wire_counts[1]), 0x5A, np.uint8)
    zv = np.full((B, c.wire_counts[0]), 0x5A5A5A5A5A5A5A5A, np.uint64)
    p = lambda a: a.ctypes.data_as(C.c_void_p) if a.size else None  # noqa: E731
    rc = _lib.lib().rv_evaluate_batch(c.ctx.handle, c.handle, C.c_size_t(B), p(w2), C.c_size_t(w2.shape[1]), p(w64), C.c_size_t(w64.shape[1]),
                                      p(gv) if gf2 else None, p(zv) if z64 else None, st.ctypes.data_as(C.c_void_p))
    assert rc == 0
    return st, gv, zv


@pytest.mark.parametrize("walk", [False, True])
def test_output_layouts_and_wide_witness_rows(rv, walk):
    B = 70
    rng = np.random.default_rng(70 + walk)
    if walk:
        prog, wc, n2, n64 = mixed_deep(14)[:4]
    else:
        prog, wc, n2, n64 = wide_mixed(layers=4, w2=4096, w64=1024, n_b2a=4)
    # rows wider than the Inputs consume, junk in the unused columns; GF(2) bytes 2, 0x80, 0xFF count as 1
    w2 = rng.choice(np.array([0, 1, 2, 0x80, 0xFF], np.uint8), (B, n2 + 5))
    w64 = rng.integers(0, 1 << 64, (B, n64 + 3), dtype=np.uint64)
    ctrl2, ctrl64 = (list(range(8)), list(range(4))) if walk else (list(range(n2 - 8, n2)), list(range(n64 - 8, n64)))
    w2[:, ctrl2] = 0
    w64[:, ctrl64] = 0
    w2[::3, ctrl2] = rng.choice(np.array([1, 2, 0x80, 0xFF], np.uint8), (len(w2[::3]), len(ctrl2)))
    w64[1::4, ctrl64] = rng.integers(1, 1 << 64, (len(w64[1::4]), len(ctrl64)), dtype=np.uint64)
    g, z, nf, ff = eval_ref.evaluate(prog, wc, w2[:, :n2], w64[:, :n64])
    assert 0 < (nf > 0).sum() < B
    c = rv.Circuit(prog, wc, keep_wires=True)
    s0 = schedules()
    calls = {(a, b): _raw(c, w2, w64, a, b) for a in (True, False) for b in (True, False)}
    s1 = schedules()
    assert s1[walk] - s0[walk] == 4 and s1[1 - walk] == s0[1 - walk]
    want_st = np.stack([nf.astype(np.uint64), ff.astype(np.int64).view(np.uint64)], axis=1)
    for (a, b), (st, gv, zv) in calls.items():
        assert np.array_equal(st, want_st), (a, b)
        assert np.array_equal(gv, g) if a else (gv == 0x5A).all(), (a, b)
        assert np.array_equal(zv, z) if b else (zv == 0x5A5A5A5A5A5A5A5A).all(), (a, b)


def _degenerate():
    return [
        ("no ops", np.zeros(0, OP_DTYPE), (3, 5), 0, 0),
        ("constants", program([SizeHint(3, 6), GF2.Const(1, 1), Z64.Const(0, 7), GF2.AddConst(2, 1, 1), GF2.MulConst(4, 1, 1)]), (3, 6), 0, 0),
        ("one level", program([GF2.Input(0), GF2.Input(1), GF2.Const(3, 1), Z64.Input(0), Z64.Input(1), Z64.Const(2, 9)]), (3, 8), 2, 2),
        ("z64 only", zb.chain_z64(lanes=3, rounds=5)[0], zb.chain_z64(lanes=3, rounds=5)[2], 0, 3),
        ("unwritten", program([GF2.Input(7), GF2.Input(3), GF2.Mul(9, 7, 3), GF2.Add(11, 9, 20), Z64.Input(2), Z64.MulConst(5, 2, 3),
                               Z64.Add(6, 5, 1), Z64.AssertZero(6)]), (9, 40), 2, 1),
    ]


@pytest.mark.parametrize("B", [1, 40])
def test_degenerate_circuits(rv, monkeypatch, B):
    rng = np.random.default_rng(B)
    for name, prog, wc, n2, n64 in _degenerate():
        c = rv.Circuit(prog, wc, keep_wires=True)
        levels = c.info["levels"]
        if name == "one level":
            assert levels == 1
        w2 = rng.choice(np.array([0, 1, 2, 0x80, 0xFF], np.uint8), (B, n2))
        w64 = rng.integers(0, 4, (B, n64), dtype=np.uint64)
        ref = eval_ref.evaluate(prog, wc, w2, w64)
        run(c, w2, w64, ref, WALK if levels >= 2 else PER_LEVEL, monkeypatch)
