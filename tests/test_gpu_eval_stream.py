"""Streaming cleartext evaluation (rv_eval_stream_*, StreamingEvaluator, evaluate_streaming) on the GPU.  Every case compares the
statuses and every wire value with the independent batched reference (tests/eval_ref.py) and with the resident evaluator on the whole
op list (Circuit(keep_wires=True).evaluate_batch(values=True)); feeds are cut at random points that do not align with the chunks."""
import ctypes as C

import numpy as np
import pytest

import bristol_gen
import circuits
import eval_ref
import z64_batch_circuits as zb
from reverie_amd.ops import GF2, OP_DTYPE, Z64, SizeHint, largest_wires, program
from test_gpu_eval import random_program, schedules
from test_gpu_eval_edges import same, same_as_ref, wide_mixed, wide_witness

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def rv():
    import reverie_amd

    reverie_amd.Context.default()
    return reverie_amd


def _inputs(ops):
    """(GF(2), Z64) Input ops of an op array"""
    inp = ops["opcode"] == 0
    return int(np.count_nonzero(inp & (ops["domain"] == 0))), int(np.count_nonzero(inp & (ops["domain"] == 1)))


def stream(rv, prog, wc, w2, w64, max_chunk_ops, rng, values=True, n_feeds=5):
    """StreamingEvaluator over feeds cut at random points; each feed gets the witness columns its Inputs consume
    -> (Evaluation, info)"""
    B = w2.shape[0]
    cuts = sorted(set(rng.integers(0, len(prog) + 1, n_feeds - 1).tolist()) | {0, len(prog)}) if len(prog) else [0, 0]
    se = rv.StreamingEvaluator(wc, batch=B, max_chunk_ops=max_chunk_ops)
    try:
        u2 = u64 = 0
        for lo, hi in zip(cuts, cuts[1:]):
            n2, n64 = _inputs(prog[lo:hi])
            se.feed(prog[lo:hi], w2[:, u2:u2 + n2], w64[:, u64:u64 + n64])
            u2, u64 = u2 + n2, u64 + n64
        r = se.finish(values=values)
        return r, se.info
    finally:
        se.close()


def check(rv, prog, wc, w2, w64, cuts, rng, ref=None, resident=None):
    """the stream at every chunk size in `cuts` equals the reference and the resident evaluator"""
    ref = ref if ref is not None else eval_ref.evaluate(prog, wc, w2, w64)
    resident = resident if resident is not None else rv.Circuit(prog, wc, keep_wires=True).evaluate_batch(w2, w64, values=True)
    for m in cuts:
        r, info = stream(rv, prog, wc, w2, w64, m, rng)
        same_as_ref(r, ref)
        same(r, resident)
        assert info["n_ops"] == len(prog)
    return resident


def _wits(rng, B, prog):
    n2, n64 = _inputs(prog)
    return rng.integers(0, 2, (B, n2)).astype(np.uint8), rng.integers(0, 1 << 64, (B, n64), dtype=np.uint64)


def _shapes():
    rng = np.random.default_rng(5)
    out = []
    # GF(2) random circuit (a SizeHint in front), and the same with a second SizeHint in the middle of the stream
    prog, wc = random_program(rng, n_gates=500, mixed=False, p_assert=0.05)
    out.append(("gf2", prog, wc))
    ops = prog.tolist()
    mid = program([tuple(o) for o in ops[:250]] + [SizeHint(wc[0], wc[1])] + [tuple(o) for o in ops[250:]])
    out.append(("gf2_hint", mid, largest_wires(mid)))
    # Z64 chains (deep, every level Z64)
    prog, _wit, wc = zb.chain_z64(lanes=4, rounds=40)
    out.append(("z64_chain", prog, wc))
    # mixed, B2A over GF(2) wires written in earlier chunks
    prog, wc = random_program(rng, n_gates=600, mixed=True, p_assert=0.04)
    out.append(("mixed", prog, wc))
    return out


SHAPES = _shapes()


@pytest.mark.parametrize("B", [1, 31, 32, 33, 1000])
def test_shapes_batches_cuts(rv, B):
    rng = np.random.default_rng(B)
    for name, prog, wc in SHAPES:
        assert tuple(largest_wires(prog)) == tuple(wc), name  # (no SizeHint grows the store)
        w2, w64 = _wits(rng, B, prog)
        check(rv, prog, wc, w2, w64, [1, 7, 64, 4096, 0], rng)


def test_evaluate_streaming_one_call_and_one_witness(rv):
    rng = np.random.default_rng(11)
    _name, prog, wc = SHAPES[3]
    w2, w64 = _wits(rng, 1, prog)
    resident = rv.Circuit(prog, wc, keep_wires=True).evaluate_batch(w2, w64, values=True)
    info = {}
    r = rv.evaluate_streaming(prog, w2[0], w64[0], wc, max_chunk_ops=7, values=True, info=info)
    same(r, resident)
    assert info["n_ops"] == len(prog) and info["chunks"] == (len(prog) + 6) // 7
    r = rv.evaluate_streaming(prog, w2, w64, wc, values=False)  # ([1][n] rows; no values)
    assert r.gf2 is None and np.array_equal(r.first_failed_op, resident.first_failed_op)
    # 1-D feeds for a batch of one
    se = rv.StreamingEvaluator(wc, max_chunk_ops=64)
    se.feed(prog, w2[0], w64[0])
    same(se.finish(values=True), resident)
    se.close()
    se.close()  # (a second close is a no-op)


# ---------------------------------------------------------------- failing assertions
def _planted_program(asserts):
    """GF(2) Inputs 0-7 (controls) and 8-15 (ones), Z64 Inputs 0-3 (controls) and 4-7 (odd), then a chain of GF(2) gates writing wires
    16-47 and Z64 gates writing 8-15 (the inputs are never overwritten).  asserts: {op index: (domain 2 or 64, control k)} puts an
    AssertZero of ctrl_k AND / * (an input that is never zero) at that index -- it fails exactly for the witnesses that set ctrl_k."""
    ops = [GF2.Input(i) for i in range(16)] + [Z64.Input(i) for i in range(8)]
    rng = np.random.default_rng(3)
    while len(ops) < 260:
        at = len(ops)
        if at in asserts:
            dom, k = asserts[at]
            ops.append(GF2.AssertZero(50 + k) if dom == 2 else Z64.AssertZero(20 + k))
        elif at + 1 in asserts:  # the product the assertion checks
            dom, k = asserts[at + 1]
            ops.append(GF2.Mul(50 + k, k, 8 + int(rng.integers(0, 8))) if dom == 2 else Z64.Mul(20 + k, k, 4 + int(rng.integers(0, 4))))
        elif rng.random() < 0.6:
            d, a, b = 16 + int(rng.integers(0, 32)), 8 + int(rng.integers(0, 40)), 8 + int(rng.integers(0, 40))
            ops.append(GF2.Mul(d, a, b) if rng.random() < 0.5 else GF2.Add(d, a, b))
        else:
            d, a, b = 8 + int(rng.integers(0, 8)), 4 + int(rng.integers(0, 12)), 4 + int(rng.integers(0, 12))
            ops.append(Z64.AddConst(d, a, 1) if rng.random() < 0.3 else Z64.Add(d, a, b))
    prog = program(ops)
    return prog, largest_wires(prog)


def _planted_witness(rng, B, fail):
    """ones / odd words in the non-control inputs; control k of witness b set for (b, k) in fail"""
    w2 = np.zeros((B, 16), np.uint8)
    w2[:, 8:] = 1
    w64 = np.zeros((B, 8), np.uint64)
    w64[:, 4:] = rng.integers(1, 1 << 20, (B, 4), dtype=np.uint64) * 2 + 1
    for b, k in fail:
        w2[b, k] = 1
        if k < 4:
            w64[b, k] = 1
    return w2, w64


@pytest.mark.parametrize("B", [1, 33])
def test_failures_fold_to_global_op_indices(rv, B):
    rng = np.random.default_rng(40 + B)
    M = 16  # chunk k = ops [16k, 16k + 16)
    # later chunk only; two chunks; both domains in one chunk (either order)
    cases = [({200: (2, 0)}, [200], 1),
             ({41: (64, 1), 150: (2, 2)}, [41, 150], 2),
             ({99: (64, 3), 103: (2, 3)}, [99, 103], 2),
             ({99: (2, 4), 103: (64, 0)}, [99, 103], 2)]
    for asserts, where, n in cases:
        prog, wc = _planted_program(asserts)
        assert all(prog[i]["opcode"] == 8 for i in where)
        ks = sorted({k for _dom, k in asserts.values()})
        fail = [(b, k) for b in range(0, B, 2) for k in ks]
        w2, w64 = _planted_witness(rng, B, fail)
        resident = check(rv, prog, wc, w2, w64, [M, 1, 0], rng)
        assert resident.n_failed[0] == n and resident.first_failed_op[0] == where[0], (asserts, resident.first_failed_op[:2])
        if B > 1:
            assert resident.n_failed[1] == 0 and resident.first_failed_op[1] == -1


# ---------------------------------------------------------------- both schedules, poison
def test_both_schedules_and_poison(rv, monkeypatch):
    from reverie_amd import bristol

    rng = np.random.default_rng(8)
    # SHA-256 in large chunks walks
    prog, info = bristol.parse(bristol_gen.sha256_block())
    wc = info["wire_counts"]
    B = 64
    w2 = rng.integers(0, 2, (B, _inputs(prog)[0])).astype(np.uint8)
    w64 = np.zeros((B, 0), np.uint64)
    ref = eval_ref.evaluate(prog, wc, w2, w64)
    resident = rv.Circuit(prog, wc, keep_wires=True).evaluate_batch(w2, w64, values=True)
    # a wide layered circuit runs per level
    wprog, wwc, n_in2, n_in64 = wide_mixed()
    ww2, ww64 = wide_witness(rng, 40, n_in2, n_in64, fail_at={3: [1], 39: [0, 5]})
    wref = eval_ref.evaluate(wprog, wwc, ww2, ww64)
    wres = rv.Circuit(wprog, wwc, keep_wires=True).evaluate_batch(ww2, ww64, values=True)
    for poison in ("0", "1"):
        monkeypatch.setenv("RV_EVAL_POISON", poison)
        s0 = schedules()
        r, inf = stream(rv, prog, wc, w2, w64, 0, rng, n_feeds=1)
        s1 = schedules()
        assert inf["chunks"] >= 1 and (s1[0] - s0[0], s1[1] - s0[1]) == (0, inf["chunks"])
        same_as_ref(r, ref)
        same(r, resident)
        r, inf = stream(rv, wprog, wwc, ww2, ww64, 0, rng, n_feeds=1)
        s2 = schedules()
        assert inf["chunks"] >= 1 and (s2[0] - s1[0], s2[1] - s1[1]) == (inf["chunks"], 0)
        same_as_ref(r, wref)
        same(r, wres)
        # small chunks and random feeds, poisoned or not
        _name, mprog, mwc = SHAPES[3]
        mw2, mw64 = _wits(np.random.default_rng(2), 33, mprog)
        check(rv, mprog, mwc, mw2, mw64, [7, 64], rng)
    monkeypatch.delenv("RV_EVAL_POISON")


# ---------------------------------------------------------------- config 4
def test_config4_full_size(rv):
    prog, wit, wc, _st = circuits.layered_gf2()
    B = 32
    rng = np.random.default_rng(4)
    w2 = rng.integers(0, 2, (B, len(wit))).astype(np.uint8)
    w2[0] = wit
    r, info = stream(rv, prog, wc, w2, np.zeros((B, 0), np.uint64), 0, rng, values=True)
    assert info["chunks"] > 30 and info["n_ops"] == len(prog)
    g, _z, nf, ff = eval_ref.evaluate_layers(prog, wc, w2)
    assert nf[0] == 0 and r.ok[0] and r.first_failed_op[0] == -1
    assert np.array_equal(r.n_failed, nf) and np.array_equal(r.first_failed_op, ff)
    assert np.array_equal(r.gf2, g)
    del g
    resident = rv.Circuit(prog, wc, keep_wires=True).evaluate_batch(w2, np.zeros((B, 0), np.uint64), values=True)
    same(r, resident)


# ---------------------------------------------------------------- errors
def test_errors(rv):
    from reverie_amd import _lib

    def code(fn):
        with pytest.raises(_lib.ReverieError) as e:
            fn()
        return e.value.code

    # Random (either domain), a SizeHint that grows the store, a short witness; afterwards only abort
    for ops, wc, w2 in ((program([GF2.Input(0), GF2.Random(1), GF2.Add(2, 0, 1)]), (0, 3), [1]),
                        (program([Z64.Random(0)]), (1, 0), []),
                        (program([GF2.Input(0), SizeHint(0, 5)]), (0, 3), [1])):
        se = rv.StreamingEvaluator(wc, max_chunk_ops=1)
        assert code(lambda: se.feed(ops, w2)) == 8
        assert code(lambda: se.feed(program([GF2.Input(0)]), [1])) == 8
        assert code(lambda: se.finish()) == 8
        se.close()
    se = rv.StreamingEvaluator((0, 3), batch=2)
    assert code(lambda: se.feed(program([GF2.Input(0), GF2.Input(1), GF2.Mul(2, 0, 1)]), np.ones((2, 1), np.uint8))) == 2
    assert code(lambda: se.finish()) == 2
    se.close()
    se = rv.StreamingEvaluator((0, 3))
    assert code(lambda: se.feed(program([GF2.Input(7)]), [1])) == 3  # (RV_E_WIRE_OOB keeps its code)
    se.close()
    # a second finish, a feed after finish
    se = rv.StreamingEvaluator((0, 1))
    se.feed(program([GF2.Input(0)]), [1])
    r = se.finish(values=True)
    assert r.gf2.tolist() == [[1]]
    assert code(lambda: se.finish()) == 9
    se.close()
    # a wire store larger than the device: refused at begin
    h = C.c_void_p()
    ctx = rv.Context.default()
    assert _lib.lib().rv_eval_stream_begin(ctx.handle, C.c_size_t(0), C.c_size_t(1 << 29), C.c_size_t(1 << 16), C.c_size_t(0), C.byref(h)) == 6
    assert not h.value
    # nothing fed: every wire reads 0, nothing fails
    se = rv.StreamingEvaluator((3, 5), batch=3)
    r = se.finish(values=True)
    assert not r.gf2.any() and not r.z64.any() and r.ok.all() and (r.first_failed_op == -1).all()
    se.close()


# ---------------------------------------------------------------- bounded memory
def test_memory_does_not_grow_with_the_stream(rv):
    """one loop body over the same wires, repeated k and 4k times: the same wire store, no larger chunk"""
    rng = np.random.default_rng(9)
    body = []
    for _ in range(32):
        d, a, b = (int(x) for x in rng.integers(0, 24, 3))
        body.append(GF2.Mul(d, a, b) if rng.random() < 0.5 else GF2.Add(d, a, b))
        d, a, b = (int(x) for x in rng.integers(0, 6, 3))
        body.append(Z64.Mul(d, a, b) if rng.random() < 0.5 else Z64.AddConst(d, a, 3))
    head = [GF2.Input(i) for i in range(24)] + [Z64.Input(i) for i in range(6)]
    out = []
    for k in (16, 64):
        prog = program(head + body * k)
        wc = largest_wires(prog)
        w2, w64 = _wits(rng, 40, prog)
        r, info = stream(rv, prog, wc, w2, w64, 256, rng, n_feeds=1)  # (one feed: every full chunk holds the same ops)
        same(r, rv.Circuit(prog, wc, keep_wires=True).evaluate_batch(w2, w64, values=True))
        out.append(info)
    assert out[0]["wire_store_bytes"] == out[1]["wire_store_bytes"] == 24 * 2 * 4 + 7 * 40 * 8 + 40 * 28
    assert out[1]["peak_chunk_bytes"] <= out[0]["peak_chunk_bytes"]
    assert out[1]["chunks"] > 3 * out[0]["chunks"] - 4


# ---------------------------------------------------------------- the CLI
def test_cli_oneshot_stream_matches_gpu(rv, tmp_path, capsys):
    from reverie_amd.__main__ import main

    from reverie_amd.ops import B2A

    ops = [GF2.Input(i) for i in range(64)] + [B2A(0, 0), Z64.Const(1, 5), Z64.Mul(2, 0, 1), Z64.SubConst(3, 2, 5 * 6),
                                              Z64.AssertZero(3)]
    p = tmp_path / "m.rvops"
    p.write_bytes(program(ops).tobytes())
    w = tmp_path / "w.txt"
    for x in (6, 7):
        w.write_text("\n".join(str((x >> i) & 1) for i in range(64)) + "\n")
        outs = []
        for extra in (["--evaluator", "gpu"], ["--evaluator", "stream"], ["--evaluator", "stream", "--max-chunk-ops", "3"]):
            argv = ["--operation", "oneshot", "--program-path", str(p), "--witness-path", str(w)] + extra
            try:
                outs.append(("rc", main(argv), capsys.readouterr().out))
            except SystemExit as e:
                outs.append(("exit", str(e), capsys.readouterr().out))
        assert outs[0] == outs[1] == outs[2], outs
        assert outs[0][0] == ("rc" if x == 6 else "exit")
    # a Bristol file goes through the same evaluator (read whole)
    bp = tmp_path / "adder.txt"
    bp.write_text(bristol_gen.adder64())
    x, y = 12345, 67890
    w.write_text("\n".join(str(b) for b in [(x >> i) & 1 for i in range(64)] + [(y >> i) & 1 for i in range(64)]) + "\n")
    e_path = tmp_path / "e.txt"
    e_path.write_text("\n".join(str(((x + y) >> i) & 1) for i in range(64)) + "\n")
    assert main(["--operation", "oneshot", "--evaluator", "stream", "--program-path", str(bp), "--witness-path", str(w),
                 "--expected-outputs-path", str(e_path)]) == 0
    e_path.write_text("\n".join(str(((x + y + 1) >> i) & 1) for i in range(64)) + "\n")
    with pytest.raises(SystemExit):
        main(["--operation", "oneshot", "--evaluator", "stream", "--program-path", str(bp), "--witness-path", str(w),
              "--expected-outputs-path", str(e_path)])
