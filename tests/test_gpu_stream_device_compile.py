"""The device compiler in the streams (RV_COMPILE_DEVICE on rv_stream_* / rv_eval_stream_*, csrc/compile_dev.hip's chunk mode).  Every
case compares against the host path or rv_prove, never against the device path itself: a piece compiled as a chunk on the GPU is the
host compiler's chunk field by field, what the device path hands back gets the host compiler's status, and the streaming prover,
verifier, batches and evaluator give the same bytes, answers and values with the flag as without it."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import circuits
from conftest import GOLDEN
from reverie_amd.ops import B2A, GF2, OP_DTYPE, SizeHint, Z64, program

pytestmark = pytest.mark.gpu

META = json.load(open(os.path.join(GOLDEN, "proofs.json")))
SMALL_GOLDEN = sorted(n for n in META if not META[n].get("digest_only"))  # (as tests/test_gpu_stream.py)


@pytest.fixture(scope="module")
def rv():
    import reverie_amd

    reverie_amd.Context.default()
    return reverie_amd


def _L():
    from reverie_amd import _lib

    return _lib.lib()


def device_chunks():
    return int(_L().rv_hook_stream_device_chunks())


def compare_chunk(prog, wc, start):
    """-> (host status, path, diff) of rv_hook_compile_compare_device_chunk; start = (mask_phase, mask64_phase, on0, pre0, on64, pre64)"""
    import reverie_amd

    prog = np.ascontiguousarray(prog)
    path, diff = C.c_int(-1), C.c_int(-1)
    rc = _L().rv_hook_compile_compare_device_chunk(reverie_amd.Context.default().handle, prog.ctypes.data_as(C.c_void_p) if len(prog) else None,
                                                   len(prog), wc[0], wc[1], (C.c_uint64 * 6)(*[int(x) for x in start]), C.byref(path), C.byref(diff))
    return rc, path.value, diff.value


def start_after(prefix):
    """the ChunkStart of the piece that follows `prefix` (all GF(2)): ShareGen calls modulo 128, online and preprocessing rows"""
    opc = prefix["opcode"]
    n_in, n_rnd, n_mul, n_as = (int((opc == k).sum()) for k in (0, 1, 6, 9))
    return ((n_in + n_rnd + 2 * n_mul) % 128, 0, n_in + n_mul + n_as, n_mul, 0, 0)


def random_programs():  # (the generator and sizes of tests/test_gpu_compile_device.py)
    rng = np.random.default_rng(0xC0DE)
    progs = []
    for k in range(240):
        n_wires = int(rng.choice([3, 6, 12, 40, 150, 600]))
        n_gates = int(rng.choice([20, 120, 400, 1500, 4000]))
        progs.append(circuits.random_gf2(rng, n_in=int(rng.integers(1, 24)), n_gates=n_gates, n_wires=n_wires))
    return progs


def _hinted(prog, wc):
    hint = prog[prog["domain"] == 3]  # a stream's wire store is sized at begin: SizeHint ops must fit in it
    return (max([wc[0]] + [int(x) for x in hint["a"]]), max([wc[1]] + [int(x) for x in hint["b"]]))


def _pieces(prog, w2, w64, cuts):
    """split (prog, witness) at the op indices `cuts`: every piece gets the witness elements its Input gates consume"""
    out = []
    i2 = i64 = 0
    edges = [0] + sorted(set(int(c) for c in cuts if 0 < c < len(prog))) + [len(prog)]
    for a, b in zip(edges[:-1], edges[1:]):
        part = prog[a:b]
        n2 = int(((part["domain"] == 0) & (part["opcode"] == 0)).sum())
        n64 = int(((part["domain"] == 1) & (part["opcode"] == 0)).sum())
        out.append((part, list(w2[i2:i2 + n2]), list(w64[i64:i64 + n64])))
        i2 += n2
        i64 += n64
    return out


def _all_gf2(part):
    """a piece the device path takes (an empty feed has no piece)"""
    return len(part) > 0 and bool((part["domain"] == 0).all())


def _edges(prog, cuts):
    e = [0] + sorted(set(int(c) for c in cuts if 0 < c < len(prog))) + [len(prog)]
    return list(zip(e[:-1], e[1:]))


def _stream(prog, w2, w64, wc, seeds, cuts1, cuts2=None, same_cuts=False, device_compile=True, max_chunk_ops=0):
    from reverie_amd.stream import StreamingProver

    sp = StreamingProver(wc, seeds=seeds, max_chunk_ops=max_chunk_ops, device_compile=device_compile)
    try:
        if same_cuts:
            sp.same_cuts()
        for part, a, b in _pieces(prog, w2, w64, cuts1):
            sp.feed(part, a, b)
        comm = sp.commit()
        for part, a, b in _pieces(prog, w2, w64, cuts1 if cuts2 is None else cuts2):
            sp.feed(part, a, b)
        proof = sp.finish()
        info = sp.info
    finally:
        sp.close()
    assert proof.comm == comm
    return proof, info


# ---- 1. the chunk compile is the host compiler's ----
def test_chunk_random_programs_identical():
    rng = np.random.default_rng(0xC4A2)
    n_dev = 0
    for k, (prog, wit, wc) in enumerate(random_programs()):
        cut = int(rng.integers(0, len(prog) + 1))
        piece = prog[cut:]
        starts = [start_after(prog[:cut])] + [(ph, 0, int(rng.integers(1, 1024)), int(rng.integers(1, 1024)), 0, 0) for ph in (0, 1, 127)]
        for start in starts:
            rc, path, diff = compare_chunk(piece, wc, start)
            assert (rc, path, diff) == (0, 1, 0), (k, cut, start, rc, path, diff)
        n_dev += 1
    assert n_dev >= 200


@pytest.mark.parametrize("recycle", [False, True])
@pytest.mark.parametrize("p_and", [0.5, 1.0])
def test_chunk_layered_identical(recycle, p_and):
    prog, wit, wc, _ = circuits.layered_gf2(n_in=512, width=8192, layers=24, p_and=p_and, fold_to=128, recycle=recycle)
    n = len(prog)
    edges = [0, n // 4, n // 2, 3 * n // 4, n]
    for a, b in zip(edges[:-1], edges[1:]):
        assert compare_chunk(prog[a:b], wc, start_after(prog[:a])) == (0, 1, 0), (a, b)


HAND_PIECES = {
    "swap": [GF2.AddConst(5, 0, 0), GF2.AddConst(0, 1, 0), GF2.AddConst(1, 5, 0)],
    "swap_via_mulconst": [GF2.MulConst(5, 0, 1), GF2.MulConst(0, 1, 1), GF2.MulConst(1, 5, 1), GF2.AddConst(2, 3, 1)],
    "copy_of_carried": [GF2.AddConst(3, 2, 0)],
    "copy_of_carried_flipped": [GF2.AddConst(3, 2, 1), GF2.Mul(4, 3, 2)],
    "x_plus_x": [GF2.Add(3, 2, 2), GF2.Sub(4, 1, 1), GF2.AssertZero(3)],
    "constant_over_wire": [GF2.Const(2, 1), GF2.Const(3, 0), GF2.Mul(4, 2, 3)],
    "written_twice": [GF2.Add(3, 0, 1), GF2.Add(3, 3, 2), GF2.Mul(3, 3, 3), GF2.Add(3, 3, 0)],
    "assert_and_random_on_carried": [GF2.AssertZero(0), GF2.Random(1), GF2.AssertZero(1), GF2.Add(2, 1, 0), GF2.AssertZero(2)],
    "linear_only": [GF2.Add(4, 0, 1), GF2.AddConst(5, 4, 1), GF2.Sub(6, 5, 2), GF2.MulConst(7, 6, 0), GF2.MulConst(0, 6, 1), GF2.Const(1, 1),
                    GF2.Add(2, 1, 0)],
    "prg_plus_carried": [GF2.Input(4), GF2.Add(5, 4, 0), GF2.Add(6, 0, 4), GF2.Mul(7, 5, 6), GF2.Add(0, 7, 1)],
    "asserts_only": [GF2.AssertZero(0), GF2.AssertZero(3)],
    "empty": [],
}


@pytest.mark.parametrize("name", sorted(HAND_PIECES))
def test_chunk_hand_written_pieces(name):
    ops = HAND_PIECES[name]
    prog = program(ops) if ops else np.zeros(0, OP_DTYPE)
    for start in [(0, 0, 0, 0, 0, 0), (127, 0, 5, 3, 0, 0), (1, 1, 1000, 999, 16, 2)]:
        for wc in [(0, 8), (3, 8)]:
            assert compare_chunk(prog, wc, start) == (0, 1, 0), (name, start, wc)


# ---- 2. what the device path hands back ----
def test_chunk_fallbacks():
    base = [GF2.Input(0), GF2.Input(1), GF2.Mul(2, 0, 1)]
    bad_opcode = program(base + [GF2.Add(3, 0, 1)])
    bad_opcode["opcode"][3] = 77
    cases = {
        "z64": (program(base + [Z64.Input(0)]), 0),
        "b2a": (program([GF2.Input(i) for i in range(64)] + [B2A(0, 0)]), 0),
        "sizehint": (program(base + [SizeHint(2, 6)]), 0),
        "wire_oob": (program(base + [GF2.Add(70, 0, 1)]), 3),
        "bad_opcode": (bad_opcode, None),
    }
    for name, (prog, want) in cases.items():
        rc, path, diff = compare_chunk(prog, (2, 66), (3, 1, 7, 2, 0, 0))
        assert (path, diff) == (0, 0), (name, rc, path, diff)
        if want is not None:
            assert rc == want, (name, rc)
        else:
            assert rc != 0, name


# ---- 3. the prover ----
@pytest.mark.parametrize("name", SMALL_GOLDEN)
def test_prover_golden(rv, rule_seeds, name):
    m = META[name]
    prog = program([tuple(o) for o in m["ops"]]) if m["ops"] else np.zeros(0, OP_DTYPE)
    w2, w64 = m["wit_gf2"], [int(x) for x in m["wit_z64"]]
    wc = _hinted(prog, tuple(m["wire_counts"]))
    want = bytes(rv.Proof.new(prog, w2, w64, wc, seeds=rule_seeds))
    n = len(prog)
    for cuts in (list(range(1, n, 3)), list(range(7, n, 50)), [n // 2]):
        pieces = _pieces(prog, w2, w64, cuts)
        n_gf2 = sum(_all_gf2(p[0]) for p in pieces)
        before = device_chunks()
        proof, _ = _stream(prog, w2, w64, wc, rule_seeds, cuts)
        assert bytes(proof) == want, (name, cuts[:4])
        # both passes compile (nothing is kept without rv_stream_same_cuts); pass 2 takes pass 1's compiled chunks from the host cache
        assert device_chunks() - before == n_gf2, (name, cuts[:4])
        before = device_chunks()
        proof, _ = _stream(prog, w2, w64, wc, rule_seeds, cuts, device_compile=False)
        assert bytes(proof) == want and device_chunks() == before


@pytest.mark.parametrize("seed", range(4))
def test_prover_random_mixed(rv, seed):
    """GF(2) + Z64 + B2A: device and host pieces alternate, different cuts in the two passes"""
    rng = np.random.default_rng(5200 + seed)
    prog, w2, w64, wc = circuits.random_mixed(rng, n_gates=int(rng.integers(150, 700)))
    wc = _hinted(prog, wc)
    seeds = rng.integers(0, 256, (256, 16), dtype=np.uint8)
    want = bytes(rv.Proof.new(prog, w2, w64, wc, seeds=seeds))
    n = len(prog)
    for k in (2, 9, 30):
        c1, c2 = rng.integers(1, n, k), rng.integers(1, n, k + 1)
        # (a pass-2 piece with the position and length of a pass-1 piece comes out of pass 1's cache of compiled chunks)
        e1, e2 = _edges(prog, c1), _edges(prog, c2)
        n_gf2 = sum(_all_gf2(prog[a:b]) for a, b in e1) + sum(_all_gf2(prog[a:b]) for a, b in e2 if (a, b) not in e1)
        before = device_chunks()
        proof, info = _stream(prog, w2, w64, wc, seeds, c1, c2)
        assert bytes(proof) == want, (seed, k)
        assert device_chunks() - before == n_gf2, (seed, k)
        assert info["n_ops"] == n


@pytest.mark.parametrize("threads", ["1", "4"])
@pytest.mark.parametrize("keep_mb", ["0", "1", None])
def test_prover_kept_transcripts_and_threads(rv, rule_seeds, monkeypatch, threads, keep_mb):
    from reverie_amd.stream import prove_streaming

    monkeypatch.setenv("RV_STREAM_THREADS", threads)
    if keep_mb is None:
        monkeypatch.delenv("RV_STREAM_KEEP_MB", raising=False)
    else:
        monkeypatch.setenv("RV_STREAM_KEEP_MB", keep_mb)
    rng = np.random.default_rng(77)
    prog, wit, wc = circuits.random_gf2(rng, n_in=60, n_gates=30000, n_wires=400, p_assert=0.0)
    want = bytes(rv.Proof.new(prog, wit, [], wc, seeds=rule_seeds))
    n_pieces = -(-len(prog) // 2048)
    before = device_chunks()
    proof, info = prove_streaming(prog, wit, [], wc, seeds=rule_seeds, max_chunk_ops=2048, device_compile=True)
    assert bytes(proof) == want
    assert info["chunks"] >= n_pieces
    assert device_chunks() - before == n_pieces  # (pass 2: pass 1's compiled chunks, or its kept transcripts)
    before = device_chunks()
    proof, _ = prove_streaming(prog, wit, [], wc, seeds=rule_seeds, max_chunk_ops=2048)
    assert bytes(proof) == want and device_chunks() == before
    # the same with cuts of the caller's and the promise to repeat them
    cuts = list(range(1500, len(prog), 1500))
    proof, _ = _stream(prog, wit, [], wc, rule_seeds, cuts, same_cuts=True)
    assert bytes(proof) == want


def _error_of(rv, f):
    try:
        f()
    except rv.ReverieError as e:
        return e.code
    return 0


@pytest.mark.parametrize("device_compile", [False, True])
def test_prover_errors_as_the_host_path(rv, rule_seeds, device_compile):
    from reverie_amd.stream import StreamingProver

    prog = program([GF2.Input(0), GF2.Input(1), GF2.Mul(2, 0, 1), GF2.AddConst(3, 2, 1), GF2.AssertZero(3)])
    want = {"assert": 1, "short": 2, "oob": 3, "pass2": 9}
    sp = StreamingProver((0, 4), seeds=rule_seeds, device_compile=device_compile)
    assert _error_of(rv, lambda: sp.feed(prog, [1, 0], [])) == want["assert"]
    sp.close()
    sp = StreamingProver((0, 4), seeds=rule_seeds, device_compile=device_compile)
    assert _error_of(rv, lambda: sp.feed(prog, [1], [])) == want["short"]
    sp.close()
    sp = StreamingProver((0, 3), seeds=rule_seeds, device_compile=device_compile)
    assert _error_of(rv, lambda: sp.feed(prog, [1, 1], [])) == want["oob"]
    sp.close()
    other = prog.copy()
    other["a"][2] = 1  # pass 2 is fed other ops of the same shape
    sp = StreamingProver((0, 4), seeds=rule_seeds, device_compile=device_compile)
    sp.feed(prog, [1, 1], [])
    sp.commit()
    sp.feed(other, [1, 1], [])
    assert _error_of(rv, sp.finish) == want["pass2"]
    sp.close()
    # the setter: only before the first feed, only the one bit
    sp = StreamingProver((0, 4), seeds=rule_seeds)
    assert _L().rv_stream_set_compile_flags(sp.handle, 8) == 9
    assert _L().rv_stream_set_compile_flags(sp.handle, 4) == 0
    sp.feed(prog, [1, 1], [])
    assert _L().rv_stream_set_compile_flags(sp.handle, 0) == 9
    sp.close()


# ---- 4. the verifier ----
@pytest.mark.parametrize("seed", range(3))
def test_verifier_matches_resident_verifier(rv, seed):
    from reverie_amd.stream import verify_streaming

    rng = np.random.default_rng(8800 + seed)
    prog, w2, w64, wc = circuits.random_mixed(rng, n_gates=int(rng.integers(150, 600)))
    wc = _hinted(prog, wc)
    seeds = rng.integers(0, 256, (256, 16), dtype=np.uint8)
    proof = rv.Proof.new(prog, w2, w64, wc, seeds=seeds)
    gprog, gwit, gwc = circuits.random_gf2(rng, n_in=30, n_gates=2500, n_wires=90)
    gproof = rv.Proof.new(gprog, gwit, [], gwc, seeds=seeds)
    for p, pr, c in ((prog, proof, wc), (gprog, gproof, gwc)):
        for strict in (True, False):
            before = device_chunks()
            ok, info = verify_streaming(p, c, pr, strict=strict, max_chunk_ops=1024, device_compile=True)
            assert ok is True and info["n_ops"] == len(p)
            if _all_gf2(p):
                assert device_chunks() - before == -(-len(p) // 1024)
        data = bytes(pr)
        for _ in range(12):
            bad = bytearray(data)
            at = int(rng.integers(0, len(bad)))
            bad[at] ^= 1 << int(rng.integers(0, 8))
            for strict in (True, False):
                try:
                    want = rv.Proof(bytes(bad)).verify(p, c, strict=strict)
                except rv.ReverieError as e:
                    want = ("err", e.code)
                try:
                    got = verify_streaming(p, c, bytes(bad), strict=strict, max_chunk_ops=1024, device_compile=True)[0]
                except rv.ReverieError as e:
                    got = ("err", e.code)
                assert got == want, (seed, at, strict)


# ---- 5. batches ----
def test_batches(rv):
    from reverie_amd.stream import prove_streaming_batch, verify_streaming_batch

    rng = np.random.default_rng(99)
    prog, wit, wc = circuits.random_gf2(rng, n_in=40, n_gates=6000, n_wires=150, p_assert=0.0)
    B = 3
    wits = np.array([[b ^ ((i + k) % 2 if k else 0) for i, b in enumerate(wit)] for k in range(B)], np.uint8)
    seeds = rng.integers(0, 256, (B, 256, 16), dtype=np.uint8)
    want = [bytes(rv.Proof.new(prog, list(wits[b]), [], wc, seeds=seeds[b])) for b in range(B)]
    before = device_chunks()
    proofs = prove_streaming_batch(prog, wits, [], wc, seeds=seeds, max_chunk_ops=1024, device_compile=True)
    assert [bytes(p) for p in proofs] == want
    assert device_chunks() - before == -(-len(prog) // 1024)  # (each piece is compiled once for the whole batch)
    assert verify_streaming_batch(prog, wc, proofs, max_chunk_ops=1024, device_compile=True) == [True] * B
    bad = bytearray(want[1])
    bad[len(bad) // 2] ^= 4
    got = verify_streaming_batch(prog, wc, [want[0], bytes(bad), want[2]], max_chunk_ops=1024, device_compile=True)
    assert got == verify_streaming_batch(prog, wc, [want[0], bytes(bad), want[2]], max_chunk_ops=1024)


# ---- 6. the evaluator ----
@pytest.mark.parametrize("batch", [1, 4])
def test_evaluator(rv, batch):
    from reverie_amd.stream import evaluate_streaming
    from test_gpu_eval import random_program

    rng = np.random.default_rng(123 + batch)
    # Random-free programs (a Random wire has no cleartext value): GF(2) only without its SizeHint, and both domains with B2A bridges
    gprog, (_, g2) = random_program(rng, n_gates=5000, mixed=False)
    gprog, gwc = gprog[1:], (0, g2)
    mprog, (m64, m2) = random_program(rng, n_gates=600, mixed=True)
    mwc = (m64, m2)
    n_in = lambda p, dom: int(((p["domain"] == dom) & (p["opcode"] == 0)).sum())
    gwit, mw2 = rng.integers(0, 2, n_in(gprog, 0)), rng.integers(0, 2, n_in(mprog, 0))
    mw64 = rng.integers(0, 1 << 63, n_in(mprog, 1), dtype=np.uint64)
    for prog, w2, w64, wc in ((gprog, gwit, [], gwc), (mprog, mw2, mw64, mwc)):
        g = np.tile(np.asarray(w2, np.uint8), (batch, 1))
        z = np.tile(np.asarray(w64, np.uint64), (batch, 1))
        if batch > 1 and g.shape[1]:
            g[1] ^= 1  # a failing witness (or at least another one)
        if batch == 1:
            g, z = g[0], z[0]
        want = evaluate_streaming(prog, g, z, wc, max_chunk_ops=1024, values=True)
        before = device_chunks()
        got = evaluate_streaming(prog, g, z, wc, max_chunk_ops=1024, values=True, device_compile=True)
        if _all_gf2(prog):
            assert device_chunks() - before == -(-len(prog) // 1024)
        assert np.array_equal(got.ok, want.ok) and np.array_equal(got.n_failed, want.n_failed)
        assert np.array_equal(got.first_failed_op, want.first_failed_op)
        assert np.array_equal(got.gf2, want.gf2) and np.array_equal(got.z64, want.z64)
    # a witness that fails for certain
    prog = program([GF2.Input(0), GF2.Input(1), GF2.Mul(2, 0, 1), GF2.AssertZero(2), GF2.Add(3, 2, 0)])
    w = np.tile(np.array([1, 1], np.uint8), (batch, 1))
    w = w[0] if batch == 1 else w
    want = evaluate_streaming(prog, w, [], (0, 4), values=True)
    got = evaluate_streaming(prog, w, [], (0, 4), values=True, device_compile=True)
    assert not got.ok.any() and np.array_equal(got.first_failed_op, want.first_failed_op) and np.array_equal(got.gf2, want.gf2)


# ---- 7. full size, bounded memory ----
def test_full_size_config4(rv, rule_seeds):
    from reverie_amd.stream import prove_streaming

    prog, wit, wc, st = circuits.layered_gf2(recycle=True)
    c = rv.Circuit(prog, wc)
    want = bytes(rv.Proof.new(c, wit, [], seeds=rule_seeds))
    c.close()
    before = device_chunks()
    proof, info = prove_streaming(prog, wit, [], wc, seeds=rule_seeds, max_chunk_ops=1 << 18, device_compile=True)
    assert bytes(proof) == want
    # pass 1 compiles every piece of the library's cut (1/8, 1/4, 1/2 of a chunk, then whole chunks); pass 2 takes its openings from
    # the kept transcripts or its chunks from pass 1's cache
    n, full, at, n_pieces = len(prog), 1 << 18, 0, 0
    for part in (full // 8, full // 4, full // 2):
        at, n_pieces = at + part, n_pieces + 1
    n_pieces += -(-(n - at) // full)
    assert n >= 4 * full and device_chunks() - before == n_pieces
    assert info["wire_store_bytes"] + info["peak_chunk_bytes"] + info["hash_state_bytes"] + info["proof_bytes"] < 1 << 30


def test_layered_bounded_memory(rv, rule_seeds):
    """the two-depth comparison of test_stream_layered_bounded_memory with the flag: the footprint does not move when the circuit gets
    four times longer, and neither does the free device memory afterwards -- the compile scratch does not grow with the stream.
    Measured on an MI355X: the deeper stream leaves 62 - 64 MiB less free than the shallower one with the flag and 60 MiB without it
    (allocations come in 2 MiB steps); 41 MiB of either are the transcripts pass 1 keeps for pass 2 (RV_STREAM_KEEP_MB, default budget:
    15 and 56 MiB at the two depths), the rest the longer proof and hash trees; 8 MiB either way with the budget 0.  The compile
    scratch adds 2 - 4 MiB, so the check sits at its bound."""
    import torch

    from reverie_amd.stream import prove_streaming

    # (the resident prover's proofs first, on the default context: free memory is device-wide, and that context's arena grows with the circuit)
    cases = []
    for layers in (6, 24):
        prog, wit, wc, st = circuits.layered_gf2(layers=layers, width=16384, n_in=512, recycle=True)
        c = rv.Circuit(prog, wc)
        cases.append((prog, wit, wc, bytes(rv.Proof.new(c, wit, [], seeds=rule_seeds))))
        c.close()
    rv.Context.default().sync()
    ctx = rv.Context(0)
    infos, free = [], []
    for prog, wit, wc, want in cases:
        proof, info = prove_streaming(prog, wit, [], wc, seeds=rule_seeds, max_chunk_ops=40000, ctx=ctx, device_compile=True)
        assert bytes(proof) == want
        del proof
        ctx.sync()
        infos.append(info)
        free.append(torch.cuda.mem_get_info(0)[0])
    print("free device memory after the two streams:", free, "growth MiB:", (free[0] - free[1]) / 2**20, "kept MiB:", [i["kept_mib"] for i in infos])
    a, b = infos
    assert b["n_ops"] > 3 * a["n_ops"] and b["chunks"] > 3 * a["chunks"]
    assert b["peak_chunk_bytes"] <= 1.1 * a["peak_chunk_bytes"] and b["wire_store_bytes"] <= 1.1 * a["wire_store_bytes"]
    assert b["hash_state_bytes"] <= a["hash_state_bytes"] + 4 * 4 * 256 * 32  # a few more tree levels, nothing else
    assert free[0] - free[1] <= (64 << 20), free
    ctx.close()


# ---- 8. no leak ----
def test_cycles_bounded_memory(rv, rule_seeds):
    import torch

    from reverie_amd.stream import StreamingProver

    prog, wit, wc, _ = circuits.layered_gf2(n_in=1024, width=32768, layers=16, fold_to=128, recycle=True)
    ctx = rv.Context(0)
    free = []
    for _ in range(5):
        sp = StreamingProver(wc, seeds=rule_seeds, max_chunk_ops=65536, ctx=ctx, device_compile=True)
        sp.feed(prog, wit, [])
        sp.commit()
        sp.feed(prog, wit, [])
        proof = sp.finish()
        sp.close()
        del proof
        ctx.sync()
        free.append(torch.cuda.mem_get_info(0)[0])
    assert max(free[1:]) - min(free[1:]) <= (64 << 20), free
    ctx.close()
