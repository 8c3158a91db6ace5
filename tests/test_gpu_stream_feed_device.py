"""Streams fed from device memory (rv_stream_feed_device, rv_eval_stream_feed_device; csrc/feed_ops.inc, csrc/piece_sums.hip).  Every case
compares against the host feed of the same ops, rv_prove or the resident evaluator, never against the device feed itself: the sums
kernel equals the host loops, a device-fed stream gives the host-fed stream's bytes, answers, values and error codes, and
rv_hook_stream_op_traffic shows which op bytes moved.  Pieces are 1024 ops (the clamp's minimum), so a few thousand ops make several
pieces and a partial last one."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import circuits
from conftest import GOLDEN
from reverie_amd.ops import B2A, GF2, OP_DTYPE, Z64, program

pytestmark = pytest.mark.gpu

META = json.load(open(os.path.join(GOLDEN, "proofs.json")))
SMALL_GOLDEN = sorted(n for n in META if not META[n].get("digest_only"))  # (as tests/test_gpu_stream.py)
CHUNK = 1024
OP_BYTES = OP_DTYPE.itemsize
M64 = (1 << 64) - 1


@pytest.fixture(scope="module")
def rv():
    import reverie_amd

    reverie_amd.Context.default()
    return reverie_amd


def _L():
    from reverie_amd import _lib

    return _lib.lib()


def on_device(prog):
    """the packed records of a numpy program as a torch tensor in GPU memory ([n, 24] uint8)"""
    import torch

    return torch.from_numpy(np.ascontiguousarray(prog).view(np.uint8).reshape(-1, OP_BYTES).copy()).cuda()


def traffic():
    out = (C.c_uint64 * 2)()
    assert _L().rv_hook_stream_op_traffic(out) == 0
    return int(out[0]), int(out[1])


def device_chunks():
    return int(_L().rv_hook_stream_device_chunks())


def moved(t0):
    t1 = traffic()
    return t1[0] - t0[0], t1[1] - t0[1]


def n_pieces(n):
    return -(-n // CHUNK)


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


def _prove(prog, w2, w64, wc, seeds, cuts=(), where=("device", "device"), device_compile=False, same_cuts=False, pass2_prog=None):
    """both passes of a StreamingProver; where[k]: pass k + 1 is fed from "host" arrays or "device" tensors -> (proof, info)"""
    from reverie_amd.stream import StreamingProver

    sp = StreamingProver(wc, seeds=seeds, max_chunk_ops=CHUNK, device_compile=device_compile)
    try:
        if same_cuts:
            sp.same_cuts()
        for k, src in enumerate((prog, prog if pass2_prog is None else pass2_prog)):
            for part, a, b in _pieces(src, w2, w64, cuts):
                sp.feed(on_device(part) if where[k] == "device" else part, a, b)
            if k == 0:
                comm = sp.commit()
        proof = sp.finish()
        info = sp.info
    finally:
        sp.close()
    assert proof.comm == comm
    return proof, info


def gf2_program(seed, n_gates):
    rng = np.random.default_rng(seed)
    return circuits.random_gf2(rng, n_in=40, n_gates=n_gates, n_wires=150)


def mixed_three_pieces():
    """a GF(2) piece, a piece with Z64 ops and a B2A, a GF(2) piece: exactly 1024 ops each, then a GF(2) tail"""
    ops = [GF2.Input(i) for i in range(64)]
    w = 64
    while len(ops) < CHUNK:  # piece 0
        ops.append(GF2.Mul(w, (7 * w + 1) % 64, (11 * w + 3) % 64) if w % 3 else GF2.Add(w, w - 1, w - 2))
        w = 64 + (w - 63) % 100
    ops += [Z64.Input(0), Z64.Input(1), Z64.Mul(2, 0, 1), B2A(3, 0), Z64.Add(4, 3, 2)]  # piece 1
    while len(ops) < 2 * CHUNK:
        ops.append(GF2.Mul(170 + len(ops) % 20, len(ops) % 64, (len(ops) + 5) % 64) if len(ops) % 2 else Z64.AddConst(5, 4, len(ops)))
    while len(ops) < 3 * CHUNK + 300:  # piece 2 and a partial piece 3
        ops.append(GF2.Mul(200 + len(ops) % 30, len(ops) % 64, 170 + len(ops) % 20) if len(ops) % 4 else GF2.AddConst(231, 200 + len(ops) % 30, 1))
    rng = np.random.default_rng(77)
    return program(ops), rng.integers(0, 2, 64).tolist(), [3, 5], (6, 232)


# ---- 1. the summary kernel equals the host loops ----
def py_sums(prog, first_index):
    """ops_digest, count_masks and count_events in plain Python (valid ops only)"""
    s = [0] * 8
    for i, o in enumerate(prog.tolist()):
        dom, opc, _res, dst, a, b, imm = o
        h = ((first_index + i) * 0x9E3779B97F4A7C15) & M64
        for x in (dom | opc << 8 | dst << 32, a | b << 32, imm):
            h ^= (x + 0x9E3779B97F4A7C15 + (h << 6) + (h >> 2)) & M64
            h = (h * 0xFF51AFD7ED558CCD) & M64
            h ^= h >> 29
        s[0] = (s[0] + h) & M64
        one, mul, az = opc in (0, 1), opc == 6, opc == 8
        if dom == 0:
            s[1] += 1 if one else 2 if mul else 0
            s[3] += opc == 0
            s[4] += mul or az
            s[5] += mul
        elif dom == 1:
            s[2] += 1 if one else 2 if mul else 0
            s[6] += 1 if opc == 0 else 8 if (mul or az) else 0
            s[7] += mul
        elif dom == 2:
            s[1] += 64 + 126
            s[2] += 1
            s[4] += 127
            s[5] += 63
            s[7] += 1
    return s


def sum_programs():
    rng = np.random.default_rng(0x5075)
    gf2 = circuits.random_gf2(rng, n_in=30, n_gates=5200, n_wires=300)[0]
    mixed = np.concatenate([circuits.random_mixed(rng, n_gates=500)[0] for _ in range(3)])
    for p in (gf2, mixed):
        top = rng.random(len(p)) < 0.3
        p["imm"][top] |= np.uint64(1 << 63)  # (constants with the top bit set: the mix must not sign-extend)
    bad = mixed.copy()
    k = rng.permutation(len(bad))
    bad["opcode"][k[:400]] = rng.integers(10, 256, 400).astype(np.uint8)   # unknown opcodes ...
    bad["domain"][k[300:700]] = rng.integers(3, 256, 400).astype(np.uint8)  # ... SizeHint and unknown domains, some on the same ops
    bad["reserved"][k[600:800]] = 0xBEEF                                    # (not digested; the compiler rejects it)
    assert min(len(gf2), len(mixed)) >= 4097
    return {"gf2": gf2, "mixed": mixed, "bad": bad}


def test_piece_sums_equal_the_host_loops(rv):
    ctx = rv.Context.default().handle
    progs = sum_programs()
    seen_nonzero = [False] * 8
    for name, prog in progs.items():
        for n in (0, 1, 63, 64, 65, 1023, 1024, 1025, 4097):
            part = np.ascontiguousarray(prog[len(prog) - n:]) if n else np.zeros(0, OP_DTYPE)  # (the tail: B2A and asserts are late in a program)
            for first in (0, 2**32 - 3, 2**40):
                h, d = (C.c_uint64 * 8)(), (C.c_uint64 * 8)()
                rc = _L().rv_hook_stream_piece_sums(ctx, part.ctypes.data_as(C.c_void_p) if n else None, n, first, 0, h, d)
                assert rc == 0 and list(h) == list(d), (name, n, first, list(h), list(d))
                if n == 0:
                    assert list(d) == [0] * 8
                if name != "bad" and n in (1, 65, 1025):  # the host loops themselves, against their definition
                    assert list(h) == py_sums(part, first), (name, n, first)
                seen_nonzero = [a or bool(x) for a, x in zip(seen_nonzero, d)]
    assert all(seen_nonzero)  # every one of the eight sums was exercised


def test_piece_sums_of_a_cut_table(rv):
    """one launch over many pieces (blockIdx.y, the cut table, the rows of the sums table): every piece equals the host loops on it"""
    ctx = rv.Context.default().handle
    for name, prog in sum_programs().items():
        prog = np.ascontiguousarray(prog[:4097 + 600])
        n = len(prog)
        for piece_ops, first in ((1024, 2**32 - 3000), (65, 2**40), (1, 0), (n, 7), (n + 5, 7)):
            pieces = max(1, -(-n // piece_ops))
            h, d = (C.c_uint64 * (8 * pieces))(), (C.c_uint64 * (8 * pieces))()
            assert _L().rv_hook_stream_piece_sums(ctx, prog.ctypes.data_as(C.c_void_p), n, first, piece_ops, h, d) == 0
            h, d = np.frombuffer(h, np.uint64).reshape(pieces, 8), np.frombuffer(d, np.uint64).reshape(pieces, 8)
            assert np.array_equal(h, d), (name, piece_ops, np.nonzero((h != d).any(axis=1))[0][:5])
            if name != "bad" and piece_ops == 1024:  # the host rows against the definition, at their positions in the stream
                for i in (0, 2, pieces - 1):  # (piece 2 crosses position 2^32)
                    assert [int(x) for x in h[i]] == py_sums(prog[i * 1024:(i + 1) * 1024], first + i * 1024), (name, i)
            assert pieces == 1 or len({int(x) for x in d[:, 0]}) > pieces // 2  # (the pieces' digests differ: no row was written twice)


# ---- 2. prover parity ----
def _check_prover(rv, prog, w2, w64, wc, seeds, want):
    n = len(prog)
    all_gf2 = n > 0 and bool((prog["domain"] == 0).all())
    for cuts in ((), (n // 3, 2 * n // 3 + 1)):
        feeds = [len(p[0]) for p in _pieces(prog, w2, w64, cuts)]
        pieces = sum(n_pieces(k) for k in feeds)
        for flag in (True, False):
            t0, c0 = traffic(), device_chunks()
            proof, info = _prove(prog, w2, w64, wc, seeds, cuts, device_compile=flag)
            assert bytes(proof) == want, (cuts, flag)
            assert info["n_ops"] == n and info["chunks"] == pieces
            if not flag:  # pass 1 copies every piece down once; pass 2 finds pass 1's compiled pieces
                assert moved(t0) == (0, OP_BYTES * n) and device_chunks() == c0, (cuts, moved(t0))
            elif all_gf2:
                assert moved(t0) == (0, 0) and device_chunks() - c0 == pieces, (cuts, moved(t0))


@pytest.mark.parametrize("which", ["about_5000", "exactly_4096"])
def test_prover_random_gf2(rv, rule_seeds, which):
    prog, wit, wc = gf2_program(0xFEED, 5600)
    if which == "exactly_4096":
        prog = np.ascontiguousarray(prog[:4096])
    assert 4096 <= len(prog) < 6000 and (which != "exactly_4096" or len(prog) == 4096)
    want = bytes(rv.Proof.new(prog, wit, [], wc, seeds=rule_seeds))
    _check_prover(rv, prog, wit, [], wc, rule_seeds, want)
    # the host feed of the same stream gives the same figures
    host, hinfo = _prove(prog, wit, [], wc, rule_seeds, where=("host", "host"))
    dev, dinfo = _prove(prog, wit, [], wc, rule_seeds)
    assert bytes(host) == bytes(dev) == want and hinfo == dinfo


@pytest.mark.parametrize("name", SMALL_GOLDEN)
def test_prover_golden(rv, rule_seeds, name):
    m = META[name]
    prog = program([tuple(o) for o in m["ops"]]) if m["ops"] else np.zeros(0, OP_DTYPE)
    w2, w64 = m["wit_gf2"], [int(x) for x in m["wit_z64"]]
    wc = _hinted(prog, tuple(m["wire_counts"]))
    want = bytes(rv.Proof.new(prog, w2, w64, wc, seeds=rule_seeds))
    _check_prover(rv, prog, w2, w64, wc, rule_seeds, want)


# ---- 3. a mixed program: only what the device compiler hands back comes down ----
def test_mixed_program_copies_only_handed_back_pieces(rv, rule_seeds):
    prog, w2, w64, wc = mixed_three_pieces()
    assert bool((prog[:CHUNK]["domain"] == 0).all()) and bool((prog[2 * CHUNK:]["domain"] == 0).all()) and 2 in prog[CHUNK:2 * CHUNK]["domain"]
    host, hinfo = _prove(prog, w2, w64, wc, rule_seeds, where=("host", "host"), device_compile=True)
    t0, c0 = traffic(), device_chunks()
    dev, dinfo = _prove(prog, w2, w64, wc, rule_seeds, device_compile=True)
    assert moved(t0) == (0, OP_BYTES * CHUNK) and device_chunks() - c0 == 3  # (pieces 0, 2 and the partial 3 stay on the device)
    assert bytes(dev) == bytes(host) == bytes(rv.Proof.new(prog, w2, w64, wc, seeds=rule_seeds)) and dinfo == hinfo


# ---- 4. the passes of one stream fed from different places ----
@pytest.mark.parametrize("flag", [False, True])
def test_passes_mixed(rv, rule_seeds, flag):
    from reverie_amd.stream import StreamingProver

    prog, wit, wc = gf2_program(0xABCD, 3500)
    want = bytes(rv.Proof.new(prog, wit, [], wc, seeds=rule_seeds))
    for where in (("host", "device"), ("device", "host")):
        for same_cuts in (True, False):  # (True: rv_stream_same_cuts holds across the mix -- pass 2 is served from pass 1's kept transcripts)
            proof, _ = _prove(prog, wit, [], wc, rule_seeds, where=where, device_compile=flag, same_cuts=same_cuts)
            assert bytes(proof) == want, (where, same_cuts)
    # pass 2 from the device with one op changed: the host feed's answer, RV_E_ARG at finish
    other = prog.copy()
    k = int(np.nonzero(other["opcode"] == 6)[0][-1])  # the last Mul reads another operand: same length, same counters
    other["a"][k] = (int(other["a"][k]) + 1) % wc[1]
    codes = {}
    for src in ("host", "device"):
        with pytest.raises(rv.ReverieError) as e:
            _prove(prog, wit, [], wc, rule_seeds, where=("host", src), device_compile=flag, pass2_prog=other)
        codes[src] = e.value.code
    assert codes == {"host": 9, "device": 9}
    # host and device feeds inside one pass
    sp = StreamingProver(wc, seeds=rule_seeds, max_chunk_ops=CHUNK, device_compile=flag)
    try:
        for k in range(2):
            for j, (part, a, b) in enumerate(_pieces(prog, wit, [], (1500, 2900))):
                sp.feed(on_device(part) if (j + k) % 2 else part, a, b)
            if k == 0:
                sp.commit()
        assert bytes(sp.finish()) == want
    finally:
        sp.close()


# ---- 5. errors: the host feed's code, and the stream stays dead ----
@pytest.mark.parametrize("flag", [False, True])
def test_errors_match_the_host_feed(rv, rule_seeds, flag):
    from reverie_amd.stream import StreamingProver

    prog, wit, wc = gf2_program(0xE44, 5000)
    assert n_pieces(len(prog)) == 5
    at = 2 * CHUNK + int(np.nonzero(prog["opcode"][2 * CHUNK:3 * CHUNK] == 6)[0][10])  # a Mul in piece 3 of 5
    assert 2 * CHUNK <= at < 3 * CHUNK
    oob = prog.copy()
    oob["a"][at] = wc[1] + 7
    bad = prog.copy()
    bad["opcode"][at] = 77
    for name, p, want in (("wire_oob", oob, 3), ("bad_opcode", bad, 5)):
        got = {}
        for src in ("host", "device"):
            sp = StreamingProver(wc, seeds=rule_seeds, max_chunk_ops=CHUNK, device_compile=flag)
            try:
                with pytest.raises(rv.ReverieError) as e:
                    sp.feed(on_device(p) if src == "device" else p, wit, [])
                with pytest.raises(rv.ReverieError) as e2:  # sticky: a good feed is refused with the same code
                    sp.feed(on_device(prog[:10]) if src == "device" else prog[:10], wit, [])
                got[src] = (e.value.code, e2.value.code, str(e.value))
            finally:
                sp.close()
        assert got["host"] == got["device"] and got["device"][:2] == (want, want), (name, got)


def test_bad_op_pointers_are_error_returns_on_a_live_stream(rv, rule_seeds):
    """NULL with n_ops > 0 and a pointer that is not 8-byte aligned: RV_E_ARG before anything is read.  The prover's feed leaves the
    stream usable (as rv_stream_feed does for a NULL array); the evaluator's makes it sticky (as rv_eval_stream_feed does)."""
    from reverie_amd.stream import StreamingEvaluator, StreamingProver

    eprog, ewit, ewc, _ = circuits.layered_gf2(n_in=64, width=256, layers=8, fold_to=128)
    d_prog = on_device(eprog)
    odd = C.c_void_p(d_prog.data_ptr() + 4)
    want = bytes(rv.Proof.new(eprog, ewit, [], ewc, seeds=rule_seeds))
    sp = StreamingProver(ewc, seeds=rule_seeds, max_chunk_ops=CHUNK)
    try:
        feed = _L().rv_stream_feed_device
        assert feed(sp.handle, None, 5, None, 0, None, 0) == 9
        assert feed(sp.handle, odd, 5, None, 0, None, 0) == 9
        assert _L().rv_stream_feed(sp.handle, None, C.c_size_t(5), None, C.c_size_t(0), None, C.c_size_t(0)) == 9  # (the host feed: the same answer)
        sp.feed(d_prog, ewit, [])
        sp.commit()
        sp.feed(d_prog, ewit, [])
        assert bytes(sp.finish()) == want
    finally:
        sp.close()
    g = np.asarray(ewit, np.uint8)
    for bad in (None, odd):
        se = StreamingEvaluator(ewc, max_chunk_ops=CHUNK)
        try:
            assert _L().rv_eval_stream_feed_device(se.handle, bad, 5, None, 0, None, 0) == 9
            with pytest.raises(rv.ReverieError) as e:  # sticky
                se.feed(d_prog, g, [])
            assert e.value.code == 9
        finally:
            se.close()


# ---- 6. verifier, batches, evaluator ----
@pytest.mark.parametrize("flag", [False, True])
def test_verifier(rv, rule_seeds, flag):
    from reverie_amd.stream import StreamingVerifier

    prog, wit, wc = gf2_program(0xFEED, 5600)
    proof = bytes(rv.Proof.new(prog, wit, [], wc, seeds=rule_seeds))
    flipped = bytearray(proof)
    flipped[len(flipped) // 2] ^= 0x10
    d_prog = on_device(prog)
    for pr, strict in ((proof, True), (proof, False), (bytes(flipped), True), (bytes(flipped), False)):
        answers = {}
        for src in ("host", "device"):
            sv = StreamingVerifier(wc, pr, max_chunk_ops=CHUNK, device_compile=flag)
            try:
                t0 = traffic()
                for a, b in ((0, 2000), (2000, len(prog))):
                    sv.feed(d_prog[a:b] if src == "device" else prog[a:b])
                if src == "device":
                    assert moved(t0) == ((0, 0) if flag else (0, OP_BYTES * len(prog)))
                answers[src] = (sv.finish(strict), sv.info)
            finally:
                sv.close()
        assert answers["host"] == answers["device"], (strict, pr == proof, answers)
        if pr == proof or strict:
            assert answers["device"][0] == (pr == proof), (strict, pr == proof)


@pytest.mark.parametrize("flag", [False, True])
def test_batches(rv, rule_seeds, flag):
    from reverie_amd.stream import StreamingBatchProver, StreamingBatchVerifier

    rng = np.random.default_rng(0xBA7C)
    prog, wit, wc = circuits.random_gf2(rng, n_in=40, n_gates=2800, n_wires=150, p_assert=0.0)  # (no AssertZero: every witness is valid)
    wits = np.stack([np.asarray(wit, np.uint8), rng.integers(0, 2, len(wit)).astype(np.uint8), 1 - np.asarray(wit, np.uint8)])
    seeds = np.stack([np.roll(np.asarray(rule_seeds, np.uint8).reshape(256, 16), b, axis=0) for b in range(3)])
    want = [bytes(rv.Proof.new(prog, wits[b].tolist(), [], wc, seeds=seeds[b])) for b in range(3)]
    d_prog = on_device(prog)
    sp = StreamingBatchProver(wc, 3, seeds=seeds, max_chunk_ops=CHUNK, device_compile=flag)
    try:
        t0, c0 = traffic(), device_chunks()
        sp.feed(d_prog, wits)
        sp.commit()
        sp.feed(d_prog, wits)
        proofs = sp.finish()
        assert moved(t0) == ((0, 0) if flag else (0, OP_BYTES * len(prog)))  # (each piece once for the whole batch)
        assert device_chunks() - c0 == (n_pieces(len(prog)) if flag else 0)
    finally:
        sp.close()
    assert [bytes(p) for p in proofs] == want
    flipped = bytearray(want[1])
    flipped[len(flipped) // 3] ^= 1
    for strict in (True, False):
        answers = {}
        for src in ("host", "device"):
            sv = StreamingBatchVerifier(wc, [want[0], bytes(flipped), want[2]], max_chunk_ops=CHUNK, device_compile=flag)
            try:
                sv.feed(d_prog if src == "device" else prog)
                answers[src] = sv.finish(strict)
            finally:
                sv.close()
        assert answers["host"] == answers["device"] == [True, False, True], strict


@pytest.mark.parametrize("B", [1, 5])
def test_evaluator(rv, B):
    import test_gpu_eval_stream as tes

    rng = np.random.default_rng(600 + B)
    planted, pwc = tes._planted_program({150: (2, 2), 41: (64, 1)})  # a failing AssertZero in each domain (for the witnesses that set the control)
    cases = [(prog, wc, *tes._wits(rng, B, prog)) for _name, prog, wc in tes.SHAPES]
    cases.append((planted, pwc, *tes._planted_witness(rng, B, [(b, k) for b in range(0, B, 2) for k in (1, 2)])))
    for prog, wc, w2, w64 in cases:
        resident = rv.Circuit(prog, wc, keep_wires=True).evaluate_batch(w2, w64, values=True)
        d_prog = on_device(prog)
        for flag in (False, True):
            for m in (64, 0):
                se = rv.StreamingEvaluator(wc, batch=B, max_chunk_ops=m, device_compile=flag)
                try:
                    cut = len(prog) // 2
                    n2, n64 = tes._inputs(prog[:cut])
                    se.feed(d_prog[:cut], w2[:, :n2], w64[:, :n64])
                    se.feed(d_prog[cut:], w2[:, n2:], w64[:, n64:])
                    r = se.finish(values=True)
                    assert se.info["n_ops"] == len(prog)
                finally:
                    se.close()
                tes.same(r, resident)
    assert resident.n_failed[0] == 2 and resident.first_failed_op[0] == 41  # (the planted program: its failures were seen)


# ---- 7. Python: tensors through every class and one-shot function ----
def test_python_one_shots_and_refusals(rv, rule_seeds):
    import torch

    prog, wit, wc = gf2_program(0x9A7, 2500)
    d_prog = on_device(prog)
    want = bytes(rv.Proof.new(prog, wit, [], wc, seeds=rule_seeds))
    eprog, ewit, ewc, _ = circuits.layered_gf2(n_in=64, width=256, layers=8, fold_to=128)
    assert 2 * CHUNK < len(eprog) < 3 * CHUNK and not (eprog["opcode"] == 1).any()
    for flag in (False, True):
        proof, info = rv.prove_streaming(d_prog, wit, [], wc, seeds=rule_seeds, max_chunk_ops=CHUNK, device_compile=flag)
        assert bytes(proof) == want and info["n_ops"] == len(prog) and info["chunks"] == n_pieces(len(prog))
        ok, vinfo = rv.verify_streaming(d_prog, wc, proof, max_chunk_ops=CHUNK, device_compile=flag)
        assert ok and vinfo["n_ops"] == len(prog)
        wits = np.stack([np.asarray(wit, np.uint8)] * 2)
        pair = rv.prove_streaming_batch(d_prog, wits, [], wc, seeds=np.stack([np.asarray(rule_seeds, np.uint8).reshape(256, 16)] * 2),
                                        max_chunk_ops=CHUNK, device_compile=flag)
        assert [bytes(p) for p in pair] == [want, want]
        assert rv.verify_streaming_batch(d_prog, wc, pair, max_chunk_ops=CHUNK, device_compile=flag) == [True, True]
        einfo = {}  # (a program without Random ops: a Random wire has no cleartext value, the evaluator refuses it)
        r = rv.evaluate_streaming(on_device(eprog), ewit, [], ewc, max_chunk_ops=CHUNK, values=True, info=einfo, device_compile=flag)
        ref = rv.evaluate_streaming(eprog, ewit, [], ewc, max_chunk_ops=CHUNK, values=True)
        assert np.array_equal(r.gf2, ref.gf2) and np.array_equal(r.n_failed, ref.n_failed) and einfo["n_ops"] == len(eprog)
        assert bool(r.ok.all())
    # every layout from_device_ops takes: [n * 24] uint8, [n, 3] int64
    flat = d_prog.reshape(-1)
    words = d_prog.view(torch.int64)
    assert words.shape == (len(prog), 3)
    for t in (flat, words):
        assert bytes(rv.prove_streaming(t, wit, [], wc, seeds=rule_seeds, max_chunk_ops=CHUNK)[0]) == want
    # refusals: host memory, a wrong shape, a wrong dtype, a view that is not contiguous
    sp = rv.StreamingProver(wc, seeds=rule_seeds, max_chunk_ops=CHUNK)
    try:
        with pytest.raises(TypeError):
            sp.feed(d_prog.cpu(), wit, [])
        for t in (d_prog[:, :23], d_prog.reshape(-1)[:-1], d_prog.view(torch.int32), d_prog.t()):
            with pytest.raises(ValueError):
                sp.feed(t, wit, [])
        sp.feed(d_prog, wit, [])  # (a refused tensor never reached the stream: it is still alive)
    finally:
        sp.close()
    for fn in (lambda t: rv.verify_streaming(t, wc, want), lambda t: rv.evaluate_streaming(t, wit, [], wc),
               lambda t: rv.StreamingEvaluator(wc).feed(t, wit, []), lambda t: rv.StreamingVerifier(wc, want).feed(t)):
        with pytest.raises(TypeError):
            fn(d_prog.cpu())
        with pytest.raises(ValueError):
            fn(d_prog[:, :23])
