"""Batches over one stream (rv_stream_*_batch): B witnesses of one statement proved, or B proofs verified, over ONE fed op list.
Every proof is byte-identical to rv_prove's for its witness and seeds; every answer is the single streaming verifier's."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import circuits
from conftest import GOLDEN, ROOT
from reverie_amd.ops import GF2, OP_ASSERTZERO, OP_DTYPE, OP_INPUT, Z64, program

pytestmark = pytest.mark.gpu

META = json.load(open(os.path.join(GOLDEN, "proofs.json")))
SMALL_GOLDEN = sorted(n for n in META if not META[n].get("digest_only"))


@pytest.fixture(scope="module")
def rv():
    import reverie_amd

    reverie_amd.Context.default()
    return reverie_amd


def _seeds(rule_seeds, batch):
    """per-proof seeds derived from the rule seeds (proof 0 has the rule seeds themselves)"""
    return np.stack([((rule_seeds.astype(np.int64) + 37 * b) % 256).astype(np.uint8) for b in range(batch)])


def _wc(prog, wc):
    hint = prog[prog["domain"] == 3]  # a stream's wire store is sized at begin: SizeHint ops must fit in it
    return (max([wc[0]] + [int(x) for x in hint["a"]]), max([wc[1]] + [int(x) for x in hint["b"]]))


def _pieces(prog, W2, W64, cuts):
    """split (prog, witnesses [B][n]) at the op indices `cuts`: every piece gets the witness columns its Input gates consume"""
    out = []
    i2 = i64 = 0
    edges = [0] + sorted(set(int(c) for c in cuts if 0 < c < len(prog))) + [len(prog)]
    for a, b in zip(edges[:-1], edges[1:]):
        part = prog[a:b]
        n2 = int(((part["domain"] == 0) & (part["opcode"] == OP_INPUT)).sum())
        n64 = int(((part["domain"] == 1) & (part["opcode"] == OP_INPUT)).sum())
        out.append((part, W2[:, i2:i2 + n2], W64[:, i64:i64 + n64]))
        i2 += n2
        i64 += n64
    return out


def _batch_stream(prog, W2, W64, wc, seeds, cuts1, cuts2=None, same_cuts=False):
    from reverie_amd.stream import StreamingBatchProver

    W2 = np.asarray(W2, np.uint8).reshape(len(seeds), -1)
    W64 = np.asarray(W64, np.uint64).reshape(len(seeds), -1)
    sp = StreamingBatchProver(wc, len(seeds), seeds=seeds)
    try:
        if same_cuts:
            sp.same_cuts()
        for part, a, b in _pieces(prog, W2, W64, cuts1):
            sp.feed(part, a, b)
        comms = sp.commit()
        for part, a, b in _pieces(prog, W2, W64, cuts1 if cuts2 is None else cuts2):
            sp.feed(part, a, b)
        proofs = sp.finish()
        info = sp.info
    finally:
        sp.close()
    assert [p.comm for p in proofs] == comms
    return proofs, info


def _free_witnesses(rng, prog, batch):
    """the program without its AssertZero gates (so that any witness holds) and `batch` random witnesses for it"""
    prog = prog[prog["opcode"] != OP_ASSERTZERO] if len(prog) else prog
    n2 = int(((prog["domain"] == 0) & (prog["opcode"] == OP_INPUT)).sum())
    n64 = int(((prog["domain"] == 1) & (prog["opcode"] == OP_INPUT)).sum())
    return prog, rng.integers(0, 2, (batch, n2)).astype(np.uint8), rng.integers(0, 1 << 63, (batch, n64), dtype=np.uint64)


@pytest.mark.parametrize("name", SMALL_GOLDEN)
def test_stream_batch_golden(rv, rule_seeds, name):
    from reverie_amd.stream import prove_streaming

    m = META[name]
    prog = program([tuple(o) for o in m["ops"]]) if m["ops"] else np.zeros(0, OP_DTYPE)
    gold = open(os.path.join(GOLDEN, f"proof_{name}.bin"), "rb").read()
    w2, w64 = m["wit_gf2"], [int(x) for x in m["wit_z64"]]
    wc = _wc(prog, tuple(m["wire_counts"]))
    n = len(prog)
    seeds8 = _seeds(rule_seeds, 8)
    want = [bytes(rv.Proof.new(prog, w2, w64, wc, seeds=seeds8[b])) for b in range(8)]
    assert want[0] == gold
    single, _ = prove_streaming(prog, w2, w64, wc, seeds=rule_seeds)
    for batch in (1, 3, 8):
        W2, W64 = np.tile(np.asarray(w2, np.uint8), (batch, 1)), np.tile(np.asarray(w64, np.uint64), (batch, 1))
        for cuts in ([n // 2], list(range(1, n, 3)), list(range(7, n, 50))):
            proofs, info = _batch_stream(prog, W2, W64, wc, seeds8[:batch], cuts)
            assert [bytes(p) for p in proofs] == want[:batch], (name, batch, cuts[:4])
            assert info["n_ops"] == n
        if batch == 1:
            assert bytes(proofs[0]) == bytes(single)


@pytest.mark.parametrize("seed", range(4))
def test_stream_batch_random_mixed(rv, oracle, seed):
    """GF(2) + Z64 + B2A with wire reuse, a different witness per proof, pass 2 cut elsewhere than pass 1; proof 0 through the
    CPU oracle, every proof equal to rv_prove's and accepted"""
    from reverie_amd.stream import prove_streaming_batch

    rng = np.random.default_rng(9100 + seed)
    prog, _, _, wc = circuits.random_mixed(rng, n_gates=int(rng.integers(150, 700)))
    wc = _wc(prog, wc)
    batch = (2, 3, 5, 8)[seed]
    prog, W2, W64 = _free_witnesses(rng, prog, batch)
    seeds = rng.integers(0, 256, (batch, 256, 16), dtype=np.uint8)
    want = [bytes(rv.Proof.new(prog, W2[b], W64[b], wc, seeds=seeds[b])) for b in range(batch)]
    assert want[0] == oracle.prove(prog, W2[0].tolist(), [int(x) for x in W64[0]], wc, seeds[0])
    assert len(set(want)) == batch
    n = len(prog)
    for k in (1, 2, 9):
        proofs, info = _batch_stream(prog, W2, W64, wc, seeds, rng.integers(1, n, k), rng.integers(1, n, k + 1))
        assert [bytes(p) for p in proofs] == want, (seed, k)
        assert info["chunks"] >= 1 and info["n_ops"] == n
    assert all(p.verify(prog, wc) for p in proofs)
    info = {}
    proofs = prove_streaming_batch(prog, W2, W64, wc, seeds=seeds, max_chunk_ops=1024, info=info)
    assert [bytes(p) for p in proofs] == want and info["chunks"] == (n + 1023) // 1024


def test_stream_batch_z64_only_one_call(rv, rule_seeds):
    """a Z64-only statement through the one-call form with wits_gf2=[]: the batch comes from wits_z64"""
    from reverie_amd.stream import prove_streaming_batch

    prog = program([Z64.Input(0), Z64.Input(1), Z64.Mul(2, 0, 1), Z64.Add(3, 2, 0)])
    W64 = np.arange(6, dtype=np.uint64).reshape(3, 2) + 5
    seeds = _seeds(rule_seeds, 3)
    proofs = prove_streaming_batch(prog, [], W64, (4, 0), seeds=seeds)
    assert [bytes(p) for p in proofs] == [bytes(rv.Proof.new(prog, [], W64[b], (4, 0), seeds=seeds[b])) for b in range(3)]


def _long_program(rng):
    ops = [GF2.Input(i) for i in range(8)] + [Z64.Input(i) for i in range(3)]
    for i in range(5000):
        a, b = int(rng.integers(0, 24)), int(rng.integers(0, 24))
        d = int(rng.integers(8, 24))
        ops.append(GF2.Mul(d, a, b) if i % 3 else GF2.Add(d, a, b))
        if i % 11 == 0:
            ops.append(Z64.Mul(int(rng.integers(3, 8)), int(rng.integers(0, 8)), int(rng.integers(0, 8))))
    return program(ops)


def test_stream_batch_long_transcripts(rv, rule_seeds):
    """transcripts of several BLAKE3 chunks, cut around the 1024-event marks: tails and incremental trees cross chunk
    boundaries with different contents per proof (different witnesses and seeds)"""
    rng = np.random.default_rng(15)
    prog = _long_program(rng)
    wc, batch = (8, 24), 4
    W2 = rng.integers(0, 2, (batch, 8)).astype(np.uint8)
    W64 = rng.integers(0, 1 << 63, (batch, 3), dtype=np.uint64)
    seeds = _seeds(rule_seeds, batch)
    want = [bytes(rv.Proof.new(prog, W2[b], W64[b], wc, seeds=seeds[b])) for b in range(batch)]
    n = len(prog)
    for cuts in ([1536 + 11], [1023, 1024, 1025, 2048, 3071], list(range(100, n, 137))):
        proofs, _ = _batch_stream(prog, W2, W64, wc, seeds, cuts)
        assert [bytes(p) for p in proofs] == want, cuts[:3]


def _kept_case(keep_mb):
    rng = np.random.default_rng(818)
    prog, _, _, wc = circuits.random_mixed(rng, n_gates=2500)
    wc = _wc(prog, wc)
    prog, W2, W64 = _free_witnesses(rng, prog, 3)
    seeds = rng.integers(0, 256, (3, 256, 16), dtype=np.uint8)
    cuts = sorted(int(x) for x in rng.integers(1, len(prog), 12))
    proofs, info = _batch_stream(prog, W2, W64, wc, seeds, cuts, same_cuts=True)
    return prog, W2, W64, wc, seeds, cuts, [bytes(p) for p in proofs], info


@pytest.mark.parametrize("keep_mb", ["0", "1", None])
def test_stream_batch_kept_transcripts(rv, monkeypatch, keep_mb):
    """rv_stream_same_cuts on a batch: the last chunks' transcripts are kept for all proofs within the batch's RV_STREAM_KEEP_MB
    (0: none; 1 MiB: part of the suffix; default: all) -- the proofs are the same in all three"""
    if keep_mb is None:
        monkeypatch.delenv("RV_STREAM_KEEP_MB", raising=False)
    else:
        monkeypatch.setenv("RV_STREAM_KEEP_MB", keep_mb)
    prog, W2, W64, wc, seeds, cuts, got, info = _kept_case(keep_mb)
    want = [bytes(rv.Proof.new(prog, W2[b], W64[b], wc, seeds=seeds[b])) for b in range(3)]
    assert got == want
    if keep_mb != "1":
        assert (info["kept_mib"] == 0) == (keep_mb == "0")
    if keep_mb is None:  # a chunk of pass 2 that has to run after one that was served from kept transcripts
        with pytest.raises(rv.ReverieError) as e:
            _batch_stream(prog, W2, W64, wc, seeds, cuts, cuts[:6] + [cuts[6] + 1] + cuts[7:], same_cuts=True)
        assert e.value.code == 9


def test_stream_batch_kept_budget_in_a_fresh_process(rv):
    """the same batch with a partial budget in a child process of its own: the same proofs as with the default budget here"""
    *_, want, _ = _kept_case(None)
    code = ("import sys; sys.path[:0] = [%r, %r]; import test_gpu_stream_batch as t, reverie_amd; reverie_amd.Context.default(); "
            "r = t._kept_case('3'); print(r[-1]['kept_mib']); print(b''.join(r[-2]).hex())") % (ROOT, os.path.join(ROOT, "tests"))
    env = dict(os.environ, RV_STREAM_KEEP_MB="3")
    out = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    kept, proofs = out.stdout.split()[-2:]
    assert 0 < int(kept) and bytes.fromhex(proofs) == b"".join(want)


def test_stream_batch_errors(rv, rule_seeds):
    from reverie_amd import _lib
    from reverie_amd.stream import StreamingBatchProver, StreamingProver

    L = _lib.lib()
    prog = program([GF2.Input(0), GF2.Input(1), GF2.Mul(2, 0, 1), GF2.AddConst(3, 2, 1), GF2.AssertZero(3)])
    seeds = _seeds(rule_seeds, 3)
    good = np.ones((3, 2), np.uint8)
    # a failing AssertZero in witness 2: the feed fails, the stream stays failed, rv_last_error names the witness
    sp = StreamingBatchProver((0, 4), 3, seeds=seeds)
    bad = good.copy()
    bad[2, 1] = 0
    with pytest.raises(rv.ReverieError) as e:
        sp.feed(prog, bad)
    assert e.value.code == 1
    assert b"witness 2" in L.rv_last_error()
    with pytest.raises(rv.ReverieError):
        sp.feed(prog, good)
    sp.close()
    # pass 2 with one witness changed (still satisfying): RV_E_ARG at finish
    prog2 = program([GF2.Input(0), GF2.Input(1), GF2.Mul(2, 0, 1)])
    sp = StreamingBatchProver((0, 4), 3, seeds=seeds)
    sp.feed(prog2, good)
    sp.commit()
    other = good.copy()
    other[1, 0] = 0
    sp.feed(prog2, other)
    with pytest.raises(rv.ReverieError) as e:
        sp.finish()
    assert e.value.code == 9
    sp.close()
    # the single-proof commit / finish on a batch, and the batch forms on a verifier stream: RV_E_ARG
    sp = StreamingBatchProver((0, 4), 3, seeds=seeds)
    sp.feed(prog, good)
    assert L.rv_stream_commit(sp.handle, None) == 9
    sp.commit()
    sp.feed(prog, good)
    out, n = C.c_void_p(), C.c_size_t()
    assert L.rv_stream_finish(sp.handle, C.byref(out), C.byref(n)) == 9
    ok = C.c_int()
    assert L.rv_stream_verify_finish(sp.handle, 0, C.byref(ok)) == 9
    assert L.rv_stream_verify_finish_batch(sp.handle, 0, (C.c_int * 3)()) == 9
    proofs = sp.finish()
    sp.close()
    from reverie_amd.stream import StreamingBatchVerifier

    sv = StreamingBatchVerifier((0, 4), proofs)
    sv.feed(prog)
    assert L.rv_stream_commit_batch(sv.handle, None) == 9
    assert L.rv_stream_finish_batch(sv.handle, (C.c_void_p * 3)(), (C.c_size_t * 3)()) == 9
    assert L.rv_stream_verify_finish(sv.handle, 0, C.byref(ok)) == 9
    assert sv.finish() == [True] * 3
    sv.close()
    # an oversized batch: RV_E_NOMEM at begin, nothing allocated -- with wire counts whose ONE store fits (the check scales with B)
    import torch

    h = C.c_void_p()
    ctx = rv.Context.default()
    free_b, _ = torch.cuda.mem_get_info()
    z64 = int(0.35 * free_b) // (256 * 72)  # one Z64 wire store: 35 % of what is free
    assert L.rv_stream_begin_batch(ctx.handle, z64, 0, 1, None, 0, C.byref(h)) == 0 and h.value
    L.rv_stream_abort(h)
    h = C.c_void_p()
    assert L.rv_stream_begin_batch(ctx.handle, z64, 0, 3, None, 0, C.byref(h)) == 6
    assert not h.value
    vp = (C.c_void_p * 3)(*[C.cast(p._buffer()[0], C.c_void_p).value for p in proofs])
    vl = (C.c_size_t * 3)(*[len(p) for p in proofs])
    assert L.rv_stream_verify_begin_batch(ctx.handle, z64, 0, 3, vp, vl, 0, C.byref(h)) == 6
    assert not h.value
    assert L.rv_stream_verify_begin_batch(ctx.handle, z64, 0, 1, vp, vl, 0, C.byref(h)) == 0 and h.value
    L.rv_stream_abort(h)
    # batch == 0 with a context
    assert L.rv_stream_begin_batch(ctx.handle, 0, 4, 0, None, 0, C.byref(h)) == 9
    # nothing is left behind: the next streams on the same context work
    again, _ = _batch_stream(prog, good, np.zeros((3, 0), np.uint64), (0, 4), seeds, [2])
    assert [bytes(p) for p in again] == [bytes(p) for p in proofs]
    sp = StreamingProver((0, 4), seeds=seeds[1])
    sp.feed(prog, [1, 1])
    sp.commit()
    sp.feed(prog, [1, 1])
    assert bytes(sp.finish()) == bytes(proofs[1])
    sp.close()


def _verify_batch_stream(proofs, prog, wc, cuts, strict=True):
    from reverie_amd.stream import StreamingBatchVerifier

    sv = StreamingBatchVerifier(wc, proofs)
    edges = [0] + sorted(set(int(c) for c in cuts if 0 < c < len(prog))) + [len(prog)]
    try:
        for a, b in zip(edges[:-1], edges[1:]):
            sv.feed(prog[a:b])
        return sv.finish(strict=strict)
    finally:
        sv.close()


def _single_verdict(rv, proof, prog, wc, strict):
    from reverie_amd.stream import verify_streaming

    try:
        return verify_streaming(prog, wc, proof, strict=strict)[0]
    except rv.ReverieError as e:
        assert e.code == 4  # (malformed: False in a batch)
        return False


@pytest.mark.parametrize("name", SMALL_GOLDEN)
def test_stream_batch_verify_golden(rv, name):
    m = META[name]
    prog = program([tuple(o) for o in m["ops"]]) if m["ops"] else np.zeros(0, OP_DTYPE)
    gold = open(os.path.join(GOLDEN, f"proof_{name}.bin"), "rb").read()
    wc = _wc(prog, tuple(m["wire_counts"]))
    n = len(prog)
    for cuts in ([], [n // 2], list(range(1, n, 3))):
        assert _verify_batch_stream([gold] * 3, prog, wc, cuts) == [True] * 3
    assert _verify_batch_stream([gold], prog, wc, [n // 2]) == [True]


@pytest.mark.parametrize("seed", range(3))
def test_stream_batch_verify_fuzz(rv, rule_seeds, seed):
    """random proofs all accepted; one proof with a flipped byte is rejected alone (ok[b] == the single streaming verifier's,
    strict and reference-compatible); a truncated proof is ok[b] = 0 without an error"""
    from reverie_amd.stream import verify_streaming_batch

    rng = np.random.default_rng(7300 + seed)
    prog, _, _, wc = circuits.random_mixed(rng, n_gates=int(rng.integers(150, 500)))
    wc = _wc(prog, wc)
    batch = 4
    prog, W2, W64 = _free_witnesses(rng, prog, batch)
    seeds = rng.integers(0, 256, (batch, 256, 16), dtype=np.uint8)
    proofs = [bytes(rv.Proof.new(prog, W2[b], W64[b], wc, seeds=seeds[b])) for b in range(batch)]
    n = len(prog)
    assert _verify_batch_stream(proofs, prog, wc, rng.integers(1, n, 3)) == [True] * batch
    info = {}
    assert verify_streaming_batch(prog, wc, proofs, max_chunk_ops=1024, info=info) == [True] * batch and info["n_ops"] == n
    for _ in range(10):
        b = int(rng.integers(0, batch))
        bad = bytearray(proofs[b])
        at = int(rng.integers(0, len(bad)))
        bad[at] ^= 1 << int(rng.integers(0, 8))
        batch_proofs = proofs[:b] + [bytes(bad)] + proofs[b + 1:]
        for strict in (True, False):
            want = [True] * batch
            want[b] = _single_verdict(rv, bytes(bad), prog, wc, strict)
            assert _verify_batch_stream(batch_proofs, prog, wc, rng.integers(1, n, 3), strict=strict) == want, (seed, at, strict)
    short = proofs[:1] + [proofs[1][:len(proofs[1]) // 2], proofs[2][:20]] + proofs[3:]
    assert _verify_batch_stream(short, prog, wc, [n // 2]) == [True, False, False, True]


def test_stream_batch_verify_false_statements(rv, rule_seeds):
    """a proof of C1 checked against C2 (failing AssertZero gates, the same transcripts): refused when strict, accepted in the
    reference-compatible mode -- next to honest proofs in the same batch"""
    c1, c2, a2, a64, cwc = circuits.assert_circuits()
    seeds = _seeds(rule_seeds, 3)
    pf = [bytes(rv.Proof.new(c1, a2, a64, cwc, seeds=seeds[b])) for b in range(3)]
    for cuts in ([], [3], [5, 8]):
        assert _verify_batch_stream(pf, c1, cwc, cuts, strict=True) == [True] * 3
        assert _verify_batch_stream(pf, c2, cwc, cuts, strict=True) == [False] * 3
        assert _verify_batch_stream(pf, c2, cwc, cuts, strict=False) == [True] * 3


def test_stream_batch_full_size(rv, rule_seeds):
    """BASELINE config 4 (10^7 gates, recycled wires, 2^18-op chunks) at B = 4: every proof equals rv_prove_batch's with the same
    seeds, in device memory bounded by B wire stores + one chunk per proof + B proofs + the kept budget"""
    from reverie_amd.stream import prove_streaming, prove_streaming_batch

    prog, wit, wc, st = circuits.layered_gf2(recycle=True)
    assert st["gates"] == 10027008
    batch = 4
    W = np.tile(np.asarray(wit, np.uint8), (batch, 1))  # (the circuit ends in AssertZero gates: one witness, B seeds)
    seeds = _seeds(rule_seeds, batch)
    c = rv.Circuit(prog, wc)
    want = [bytes(p) for p in rv.Proof.new_batch(c, W, seeds=seeds)]
    c.close()
    info = {}
    proofs = prove_streaming_batch(prog, W, [], wc, seeds=seeds, max_chunk_ops=1 << 18, info=info)
    assert [bytes(p) for p in proofs] == want
    single, one = prove_streaming(prog, W[0], [], wc, seeds=seeds[0], max_chunk_ops=1 << 18)
    assert bytes(single) == want[0]
    # every proof of the batch holds what a single stream holds, and no more
    assert info["proof_bytes"] == sum(len(p) for p in want)
    for k in ("wire_store_bytes", "peak_chunk_bytes", "hash_state_bytes"):
        assert info[k] == batch * one[k], k
    assert info["wire_store_bytes"] + info["peak_chunk_bytes"] + info["hash_state_bytes"] + info["proof_bytes"] < batch * (1 << 30)
