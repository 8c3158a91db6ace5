"""Streams in device memory: witnesses read there (rv_stream_feed_wdev, rv_eval_stream_feed_wdev; the digest kernel k_wit_sums),
proofs left there (rv_stream_finish_device, _finish_batch_device), proofs verified there (rv_stream_verify_begin_device,
_begin_batch_device).  Every case compares against the host-witness / host-proof stream, rv_prove or the golden bytes of the same
statement, never the new path against itself.  Pieces are 1024 ops (the clamp's minimum): a few thousand ops make several pieces and a
partial last one."""
import ctypes as C

import numpy as np
import pytest

import proof_mutate
import test_gpu_stream_feed_device as fd
import verify_length_cases as cases
from conftest import golden_ops
from reverie_amd.ops import GF2, OP_DTYPE, program

pytestmark = pytest.mark.gpu

CHUNK = fd.CHUNK
M64 = (1 << 64) - 1
E_WITNESS_INVALID, E_WITNESS_SHORT, E_MALFORMED, E_ARG = 1, 2, 4, 9


@pytest.fixture(scope="module")
def rv():
    import reverie_amd

    reverie_amd.Context.default()
    return reverie_amd


def _L():
    from reverie_amd import _lib

    return _lib.lib()


def hook(name, n):
    out = (C.c_uint64 * n)()
    assert getattr(_L(), name)(out) == 0
    return [int(x) for x in out]


def traffic():
    return hook("rv_hook_stream_traffic", 4)


def paths():
    return hook("rv_hook_stream_verify_device_paths", 2)


def delta(now, before):
    return [a - b for a, b in zip(now, before)]


def gpu2(w2, lead=0):
    """GF(2) witness bits as a uint8 GPU tensor that starts `lead` bytes into its allocation"""
    import torch

    a = np.asarray(w2, np.uint8).reshape(-1)
    return torch.from_numpy(np.concatenate([np.zeros(lead, np.uint8), a])).cuda()[lead:]


def gpu64(w64):
    import torch

    return torch.from_numpy(np.asarray([int(x) & M64 for x in w64], np.uint64).view(np.int64).copy()).cuda()


def upload(data: bytes):
    import torch

    return torch.from_numpy(np.frombuffer(bytes(data), np.uint8).copy()).cuda()


def inputs(part):
    inp = part["opcode"] == 0
    return int((inp & (part["domain"] == 0)).sum()), int((inp & (part["domain"] == 1)).sum())


def feeds(prog, cuts):
    """[(op slice, first GF(2) input, count, first Z64 input, count)] of the stream cut at the op indices `cuts`"""
    edges = [0] + sorted(set(int(c) for c in cuts if 0 < c < len(prog))) + [len(prog)]
    out, i2, i64 = [], 0, 0
    for a, b in zip(edges[:-1], edges[1:]):
        n2, n64 = inputs(prog[a:b])
        out.append((slice(a, b), i2, n2, i64, n64))
        i2, i64 = i2 + n2, i64 + n64
    return out


def prove(prog, w2, w64, wc, seeds, cuts=((), ()), ops=("host", "host"), wit=("device", "device"), same_cuts=False, lead=0, wit2=None,
          device_out=False):
    """Both passes of a StreamingProver.  cuts[k] / ops[k] / wit[k]: how pass k + 1 is cut, and whether its ops and witnesses come from
    host arrays or GPU tensors; wit2: another witness for pass 2 -> (proof, comm, info)"""
    from reverie_amd.stream import StreamingProver

    d_prog = fd.on_device(prog) if "device" in ops else None
    sp = StreamingProver(wc, seeds=seeds, max_chunk_ops=CHUNK)
    try:
        if same_cuts:
            sp.same_cuts()
        for k in range(2):
            a2, a64 = (w2, w64) if k == 0 or wit2 is None else wit2
            g, z = (gpu2(a2, lead), gpu64(a64)) if wit[k] == "device" else (np.asarray(a2, np.uint8), np.asarray(a64, np.uint64))
            for sl, i2, n2, i64, n64 in feeds(prog, cuts[k]):
                sp.feed(d_prog[sl] if ops[k] == "device" else prog[sl], g[i2:i2 + n2], z[i64:i64 + n64])
            if k == 0:
                comm = sp.commit()
        proof = sp.finish(device=device_out)
        info = sp.info
    finally:
        sp.close()
    return proof, comm, info


def golden(name):
    m = fd.META[name]
    prog = program(golden_ops(m)) if m["ops"] else np.zeros(0, OP_DTYPE)
    return prog, m["wit_gf2"], [int(x) for x in m["wit_z64"]], fd._hinted(prog, tuple(m["wire_counts"]))


_ref = {}


def reference(rv, rule_seeds, name):
    """(prog, w2, w64, wc, rv_prove's bytes, the host-fed stream's (bytes, comm, info)) of a statement: computed once, never changed"""
    if name not in _ref:
        prog, w2, w64, wc = fd.mixed_three_pieces() if name == "mixed" else golden(name)
        want = bytes(rv.Proof.new(prog, w2, w64, wc, seeds=rule_seeds))
        proof, comm, info = prove(prog, w2, w64, wc, rule_seeds, wit=("host", "host"))
        _ref[name] = (prog, w2, w64, wc, want, (bytes(proof), comm, info))
    return _ref[name]


# ---- 1. the digest kernel against wit_digest, restated ----
def py_wit_digest(w2, first2, w64, first64):
    def mix(pos, x):
        h = (pos * 0x9E3779B97F4A7C15) & M64
        h ^= (x + 0x9E3779B97F4A7C15 + (h << 6) + (h >> 2)) & M64
        h = (h * 0xFF51AFD7ED558CCD) & M64
        return h ^ (h >> 29)

    s = 0
    for i, b in enumerate(w2):
        s += mix(2 * (first2 + i) & M64, int(b) & 1)
    for i, x in enumerate(w64):
        s += mix((2 * (first64 + i) + 1) & M64, int(x))
    return s & M64


def test_wit_sums_kernel_equals_the_host_loop(rv):
    ctx = rv.Context.default().handle
    rng = np.random.default_rng(0x317)
    seen = set()
    for n2 in (0, 1, 63, 64, 65, 255, 256, 257, 2049):
        for n64 in (0, 1, 64, 257):
            for first in (0, 7, (1 << 32) + 5):
                w2 = rng.integers(0, 256, n2).astype(np.uint8)  # (every byte value: only bit 0 counts)
                w2[:3] = [2, 0xFE, 0xFF][:n2]
                w64 = rng.integers(0, 1 << 64, n64, dtype=np.uint64)
                w64[:1] = M64
                h, d = C.c_uint64(), C.c_uint64()
                rc = _L().rv_hook_stream_wit_sums(ctx, w2.ctypes.data_as(C.c_void_p) if n2 else None, n2, first,
                                                  w64.ctypes.data_as(C.c_void_p) if n64 else None, n64, first + 3, C.byref(h), C.byref(d))
                assert rc == 0
                want = py_wit_digest(w2.tolist(), first, w64.tolist(), first + 3)
                assert h.value == want and d.value == want, (n2, n64, first)
                assert want == py_wit_digest((w2 & 1).tolist(), first, w64.tolist(), first + 3)
                seen.add(want)
    assert len(seen) > 90  # (the cases digest differently: position and value both count)


# ---- 2. prover: byte equality with the host-fed stream, rv_prove and the golden bytes ----
@pytest.mark.parametrize("name", fd.SMALL_GOLDEN + ["mixed"])
def test_prover_device_witness(rv, oracle, rule_seeds, name):
    from conftest import golden_matches

    prog, w2, w64, wc, want, (host, hcomm, hinfo) = reference(rv, rule_seeds, name)
    assert host == want
    if name != "mixed":
        assert golden_matches(oracle, name, fd.META[name], want)
    n = len(prog)
    for ops in (("host", "host"), ("device", "device")):
        for cuts in (((), ()), ((n // 3, 2 * n // 3 + 1), (n // 2,))):  # the default cuts; cuts that differ between the passes
            proof, comm, info = prove(prog, w2, w64, wc, rule_seeds, cuts=cuts, ops=ops, lead=3)
            assert bytes(proof) == want and comm == hcomm == proof.comm, (ops, cuts)
            if cuts == ((), ()):
                assert info == hinfo, ops
            else:
                assert {k: info[k] for k in ("n_ops", "gf2_masks", "z64_masks", "gf2_muls", "z64_muls", "proof_bytes")} == \
                       {k: hinfo[k] for k in ("n_ops", "gf2_masks", "z64_masks", "gf2_muls", "z64_muls", "proof_bytes")}


# ---- 3. host and device witness feeds mixed between the passes and inside one ----
def test_mixed_witness_feeds(rv, rule_seeds):
    from reverie_amd.stream import StreamingProver

    prog, w2, w64, wc, want, _ = reference(rv, rule_seeds, "mixed")
    for wit in (("host", "device"), ("device", "host")):
        for same_cuts in (False, True):
            proof, _, _ = prove(prog, w2, w64, wc, rule_seeds, wit=wit, same_cuts=same_cuts)
            assert bytes(proof) == want, (wit, same_cuts)
    sp = StreamingProver(wc, seeds=rule_seeds, max_chunk_ops=CHUNK)
    try:
        g, z = gpu2(w2), gpu64(w64)
        for k in range(2):
            for j, (sl, i2, n2, i64, n64) in enumerate(feeds(prog, (700, CHUNK + 3, 2500))):
                if (j + k) % 2:
                    sp.feed(prog[sl], g[i2:i2 + n2], z[i64:i64 + n64])
                else:
                    sp.feed(prog[sl], w2[i2:i2 + n2], w64[i64:i64 + n64])
            if k == 0:
                sp.commit()
        assert bytes(sp.finish()) == want
    finally:
        sp.close()


# ---- 4. the digest bites: pass 2 fed another witness ----
def test_altered_witness_in_pass_2_is_refused(rv, rule_seeds):
    prog, w2, w64, wc, _, _ = reference(rv, rule_seeds, "mixed")
    flip2 = list(w2)
    flip2[17] ^= 1
    other64 = [w64[0], w64[1] + 1]
    for same_cuts in (False, True):  # (True: every chunk fits the budget -- the altered element lies inside a chunk that does not run)
        for wit2 in ((flip2, w64), (w2, other64)):
            for wit in (("device", "device"), ("host", "device"), ("device", "host")):
                with pytest.raises(rv.ReverieError) as e:
                    prove(prog, w2, w64, wc, rule_seeds, wit=wit, same_cuts=same_cuts, wit2=wit2)
                assert e.value.code == E_ARG, (same_cuts, wit)
    # (the same feeds with the witness unchanged pass: test_mixed_witness_feeds)


def test_kept_chunks_do_not_run_in_pass_2(rv, rule_seeds):
    """what makes the same_cuts case above mean something: pass 2 of that stream copies no witness, so only the digest saw it"""
    prog, w2, w64, wc, want, _ = reference(rv, rule_seeds, "mixed")
    t0 = traffic()
    proof, _, info = prove(prog, w2, w64, wc, rule_seeds, same_cuts=True)
    assert bytes(proof) == want and info["kept_mib"] > 0
    assert delta(traffic(), t0)[:2] == [0, len(w2) + 8 * len(w64)]  # (pass 1 alone)


# ---- 5. errors as the host feeds' ----
def failing_program():
    """GF(2): wire 2 = w0 * w1 must be zero; padded past one piece"""
    ops = [GF2.Input(0), GF2.Input(1), GF2.Mul(2, 0, 1), GF2.AssertZero(2)]
    while len(ops) < CHUNK + 200:
        ops.append(GF2.Add(3 + len(ops) % 5, 0, 1))
    return program(ops), (0, 8)


def test_errors_match_the_host_feed(rv, rule_seeds):
    from reverie_amd import _lib
    from reverie_amd.stream import StreamingBatchProver, StreamingProver

    prog, w2, w64, wc, _, _ = reference(rv, rule_seeds, "mixed")
    # a short witness, from either side
    for g, z in ((gpu2(w2[:-1]), gpu64(w64)), (gpu2(w2), gpu64(w64[:1])), (np.asarray(w2[:-1], np.uint8), np.asarray(w64, np.uint64))):
        sp = StreamingProver(wc, seeds=rule_seeds, max_chunk_ops=CHUNK)
        try:
            with pytest.raises(rv.ReverieError) as e:
                sp.feed(prog, g, z)
            assert e.value.code == E_WITNESS_SHORT
            with pytest.raises(rv.ReverieError) as e2:  # sticky: a good feed is refused with the same code
                sp.feed(prog[:10], gpu2(w2), gpu64(w64))
            assert e2.value.code == E_WITNESS_SHORT
        finally:
            sp.close()
    # a batch whose stride is below n, and a z64 pointer off by 4 bytes: RV_E_ARG before anything runs, then only abort
    seeds3 = np.stack([np.roll(np.asarray(rule_seeds, np.uint8).reshape(256, 16), b, axis=0) for b in range(3)])
    rows2, rows64 = gpu2(np.tile(np.asarray(w2, np.uint8), 3)), gpu64(list(w64) * 4)
    good = _lib.DevWitness(rows2.data_ptr(), len(w2), len(w2), rows64.data_ptr(), len(w64), len(w64))
    for bad in (_lib.DevWitness(rows2.data_ptr(), len(w2), len(w2) - 1, rows64.data_ptr(), len(w64), len(w64)),
                _lib.DevWitness(rows2.data_ptr(), len(w2), len(w2), rows64.data_ptr() + 4, len(w64), len(w64))):
        sp = StreamingBatchProver(wc, 3, seeds=seeds3, max_chunk_ops=CHUNK)
        try:
            feed = _L().rv_stream_feed_wdev
            assert feed(sp.handle, prog.ctypes.data_as(C.c_void_p), len(prog), 0, C.byref(bad)) == E_ARG
            assert feed(sp.handle, prog.ctypes.data_as(C.c_void_p), len(prog), 0, C.byref(good)) == E_ARG  # sticky
            assert _L().rv_stream_commit_batch(sp.handle, None) == E_ARG
        finally:
            sp.close()
    # a witness that fails an AssertZero: the middle one of three, named by rv_last_error
    fprog, fwc = failing_program()
    wits = np.array([[1, 0], [1, 1], [0, 1]], np.uint8)
    codes = {}
    for src in ("host", "device"):
        sp = StreamingBatchProver(fwc, 3, seeds=seeds3, max_chunk_ops=CHUNK)
        try:
            with pytest.raises(rv.ReverieError) as e:
                sp.feed(fprog, gpu2(wits).reshape(3, 2) if src == "device" else wits, [])
            codes[src] = (e.value.code, _L().rv_last_error().decode())
            with pytest.raises(rv.ReverieError) as e2:
                sp.feed(fprog[:4], wits, [])
            assert e2.value.code == E_WITNESS_INVALID
        finally:
            sp.close()
    assert codes["host"] == codes["device"] and codes["device"][0] == E_WITNESS_INVALID and "witness 1" in codes["device"][1], codes


# ---- 6. a batch whose witnesses are rows of a wider tensor ----
def batch_case(rule_seeds):
    import torch

    prog, w2, w64, wc = fd.mixed_three_pieces()
    rng = np.random.default_rng(0xB3)
    wits2 = np.stack([np.asarray(w2, np.uint8), rng.integers(0, 2, len(w2)).astype(np.uint8), 1 - np.asarray(w2, np.uint8)])
    wits64 = np.array([w64, [M64, 1 << 63], [0, 7]], np.uint64)
    seeds = np.stack([np.roll(np.asarray(rule_seeds, np.uint8).reshape(256, 16), b, axis=0) for b in range(3)])
    wide2 = torch.full((3, len(w2) + 13), 0xEE, dtype=torch.uint8, device="cuda")
    wide64 = torch.full((3, 5), -1, dtype=torch.int64, device="cuda")
    wide2[:, :len(w2)] = torch.from_numpy(wits2).cuda()
    wide64[:, :2] = torch.from_numpy(wits64.view(np.int64).copy()).cuda()
    return prog, wc, wits2, wits64, seeds, wide2[:, :len(w2)], wide64[:, :2]


def test_batch_of_strided_rows(rv, rule_seeds):
    from reverie_amd.stream import StreamingBatchProver

    prog, wc, wits2, wits64, seeds, g, z = batch_case(rule_seeds)
    assert g.stride(0) > g.shape[1] and z.stride(0) > z.shape[1]
    want = [bytes(prove(prog, wits2[b], wits64[b], wc, seeds[b], wit=("host", "host"))[0]) for b in range(3)]
    assert want[0] == bytes(rv.Proof.new(prog, wits2[0].tolist(), [int(x) for x in wits64[0]], wc, seeds=seeds[0])) and len(set(want)) == 3
    d_prog = fd.on_device(prog)
    for ops in (prog, d_prog):
        t0 = traffic()
        sp = StreamingBatchProver(wc, 3, seeds=seeds, max_chunk_ops=CHUNK)
        try:
            for k in range(2):
                for sl, i2, n2, i64, n64 in feeds(prog, (1500,)):
                    sp.feed(ops[sl], g[:, i2:i2 + n2], z[:, i64:i64 + n64])
                if k == 0:
                    sp.commit()
            proofs = sp.finish()
        finally:
            sp.close()
        assert [bytes(p) for p in proofs] == want
        # 7. traffic: nothing went up from the host; both passes' consumed elements of every proof were taken on the device
        assert delta(traffic(), t0) == [0, (wits2.shape[1] + 8 * wits64.shape[1]) * 2 * 3, sum(len(p) for p in want), 0]
    assert [bytes(p) for p in rv.prove_streaming_batch(prog, g, z, wc, seeds=seeds, max_chunk_ops=CHUNK)] == want


# ---- 7. traffic, single stream: the roles of the two witness counters swap with the witness's place ----
def test_traffic_counts_where_the_witness_came_from(rv, rule_seeds):
    prog, w2, w64, wc, want, _ = reference(rv, rule_seeds, "mixed")
    consumed = (len(w2) + 8 * len(w64)) * 2
    t0 = traffic()
    assert bytes(prove(prog, w2, w64, wc, rule_seeds, wit=("device", "device"))[0]) == want
    assert delta(traffic(), t0) == [0, consumed, len(want), 0]
    t0 = traffic()
    assert bytes(prove(prog, w2, w64, wc, rule_seeds, wit=("host", "host"))[0]) == want
    assert delta(traffic(), t0) == [consumed, 0, len(want), 0]


# ---- 8. the proof left in device memory ----
def test_finish_device(rv, rule_seeds):
    import torch

    from reverie_amd.stream import StreamingProver

    prog, w2, w64, wc, want, _ = reference(rv, rule_seeds, "mixed")
    t0 = traffic()
    dp, comm, info = prove(prog, w2, w64, wc, rule_seeds, device_out=True)
    assert isinstance(dp, rv.DeviceProof) and delta(traffic(), t0)[2] == 0
    assert bytes(dp.tensor.cpu().numpy().tobytes()) == want and dp.comm == comm and info["proof_bytes"] == len(want)
    c = rv.Circuit(prog, wc)
    assert dp.verify(c, strict=True) is True  # rv_verify_device takes the tensor
    one_shot, _ = rv.prove_streaming(prog, gpu2(w2), gpu64(w64), wc, seeds=rule_seeds, max_chunk_ops=CHUNK, device_proof=True)
    assert bytes(one_shot.to_proof()) == want
    # the destination's checks leave the stream alive
    sp = StreamingProver(wc, seeds=rule_seeds, max_chunk_ops=CHUNK)
    try:
        for k in range(2):
            sp.feed(prog, gpu2(w2), gpu64(w64))
            if k == 0:
                sp.commit()
        buf = torch.zeros(len(want) + 64, dtype=torch.uint8, device="cuda")
        fin = _L().rv_stream_finish_device
        n = C.c_size_t()
        assert fin(sp.handle, C.c_void_p(buf.data_ptr()), len(want) - 1, C.byref(n)) == E_ARG and n.value == len(want)
        n = C.c_size_t()
        assert fin(sp.handle, C.c_void_p(buf.data_ptr() + 8), len(want), C.byref(n)) == E_ARG and n.value == len(want)
        host = np.zeros(len(want), np.uint8)
        assert fin(sp.handle, host.ctypes.data_as(C.c_void_p), len(want), C.byref(n)) == E_ARG  # not device memory
        assert not buf.any()
        assert fin(sp.handle, C.c_void_p(buf.data_ptr()), len(want), C.byref(n)) == 0 and n.value == len(want)
        assert buf[:len(want)].cpu().numpy().tobytes() == want and not buf[len(want):].any()
        assert fin(sp.handle, C.c_void_p(buf.data_ptr()), len(want), C.byref(n)) == E_ARG  # finished
    finally:
        sp.close()


def test_finish_batch_device(rv, rule_seeds):
    import torch

    from reverie_amd.stream import StreamingBatchProver, StreamingProver

    prog, wc, wits2, wits64, seeds, g, z = batch_case(rule_seeds)
    host = [bytes(p) for p in rv.prove_streaming_batch(prog, wits2, wits64, wc, seeds=seeds, max_chunk_ops=CHUNK)]
    t0 = traffic()
    views = rv.prove_streaming_batch(prog, g, z, wc, seeds=seeds, max_chunk_ops=CHUNK, device_proof=True)
    assert delta(traffic(), t0)[2] == 0
    stride = (len(host[0]) + 255) & ~255
    base = views[0].tensor.data_ptr()
    assert [v.tensor.data_ptr() - base for v in views] == [0, stride, 2 * stride]  # proof b at b * stride of one tensor
    assert [v.tensor.cpu().numpy().tobytes() for v in views] == host
    # the batch form's own rules, and the single stream it also takes
    sp = StreamingBatchProver(wc, 3, seeds=seeds, max_chunk_ops=CHUNK)
    try:
        for k in range(2):
            sp.feed(prog, g, z)
            if k == 0:
                sp.commit()
        buf = torch.zeros(3 * stride + 256, dtype=torch.uint8, device="cuda")
        fin = _L().rv_stream_finish_batch_device
        n = C.c_size_t()
        assert fin(sp.handle, C.c_void_p(buf.data_ptr()), stride - 256, C.byref(n)) == E_ARG and n.value == len(host[0])
        assert fin(sp.handle, C.c_void_p(buf.data_ptr()), stride + 16, C.byref(n)) == E_ARG
        assert fin(sp.handle, C.c_void_p(buf.data_ptr() + 16), stride, C.byref(n)) == E_ARG
        assert _L().rv_stream_finish_device(sp.handle, C.c_void_p(buf.data_ptr()), 3 * stride, C.byref(n)) == E_ARG  # the single form on a batch
        assert not buf.any()
        assert fin(sp.handle, C.c_void_p(buf.data_ptr()), stride, C.byref(n)) == 0 and n.value == len(host[0])
        assert [buf[b * stride:b * stride + n.value].cpu().numpy().tobytes() for b in range(3)] == host
    finally:
        sp.close()
    single = StreamingProver(wc, seeds=seeds[1], max_chunk_ops=CHUNK)
    try:
        for k in range(2):
            single.feed(prog, wits2[1], wits64[1])
            if k == 0:
                single.commit()
        buf = torch.zeros(len(host[1]) + 16, dtype=torch.uint8, device="cuda")
        n = C.c_size_t()
        assert _L().rv_stream_finish_batch_device(single.handle, C.c_void_p(buf.data_ptr() + 16), len(host[1]), C.byref(n)) == 0
        assert buf[16:].cpu().numpy().tobytes() == host[1]
    finally:
        single.close()


# ---- 9. the verifier begun on a proof in device memory ----
def answer(rv, prog, wc, proof, strict):
    """verify_streaming's answer or error code on host bytes or on a GPU tensor"""
    try:
        return rv.verify_streaming(prog, wc, proof, strict=strict, max_chunk_ops=CHUNK)[0]
    except rv.ReverieError as e:
        return ("error", e.code)


def both(rv, prog, wc, data, strict, path):
    """the device begin's answer next to the host form's on the same bytes; path: 0 in place, 1 the fallback"""
    p0, t0 = paths(), traffic()
    dev = answer(rv, prog, wc, upload(data), strict)
    took, up = delta(paths(), p0), delta(traffic(), t0)[3]
    assert took == ([1, 0] if path == 0 else [0, 1]), (took, path)
    assert path == 1 or up == 0  # in place: no proof byte went up from the host
    return dev, answer(rv, prog, wc, bytes(data), strict)


@pytest.mark.parametrize("name", ["gf2_mix", "adder64", "mixed"])
def test_verifier_accepts_valid_proofs_in_place(rv, rule_seeds, name):
    prog, _, _, wc, want, _ = reference(rv, rule_seeds, name)
    for strict in (True, False):
        assert both(rv, prog, wc, want, strict, 0) == (True, True)
    from reverie_amd.stream import StreamingVerifier

    d_prog = fd.on_device(prog)
    sv = StreamingVerifier(wc, rv.DeviceProof(upload(want)), max_chunk_ops=CHUNK)  # a DeviceProof, device ops, two feeds
    try:
        sv.feed(d_prog[:len(prog) // 2])
        sv.feed(d_prog[len(prog) // 2:])
        assert sv.finish() is True and sv.info["n_ops"] == len(prog)
    finally:
        sv.close()


MUTATION_PARTS = [(d, v) for d in proof_mutate.DOMAINS for v in proof_mutate.VECTORS] + [("same", None)]


@pytest.mark.parametrize("dom,vec", MUTATION_PARTS)
def test_verifier_mutations_answer_as_the_host_form(rv, rule_seeds, dom, vec):
    prog, _, _, wc, want, _ = reference(rv, rule_seeds, "mixed")
    if dom == "same":
        entries = list(proof_mutate.catalogue(want, domains=(), gf2_items=cases.gf2_items(prog)))
    else:
        entries = list(proof_mutate.catalogue(want, domains=(dom,), vectors=(vec,), same_length=False))
    assert len(entries) >= 20
    seen = set()
    for label, data in entries:
        p0 = paths()
        dev = answer(rv, prog, wc, upload(data), True)
        took = delta(paths(), p0)
        assert sum(took) == 1
        host = answer(rv, prog, wc, data, True)
        assert dev == host, (label, dev, host, took)
        seen.add((host if isinstance(host, bool) else host[0], took[0]))
    assert (False, 1) in seen or ("error", 0) in seen  # (the catalogue reached the in-place path's refusals or the fallback's)


def test_verifier_byte_flips_truncations_counts_and_batch(rv, rule_seeds):
    prog, _, _, wc, want, _ = reference(rv, rule_seeds, "mixed")
    comm, doms = proof_mutate.parse(want)
    # where a record's vectors, a preprocessing seed and comm lie in the bytes
    rec0 = 32 + 8
    pre2 = 32 + 8 + sum(1 + 128 + sum(8 + len(v) for v in r[2]) for r in doms[0][0]) + 8
    n_z = sum(1 + 128 + sum(8 + len(v) for v in r[2]) for r in doms[1][0])
    pre64 = pre2 + 216 * 48 + 8 + n_z + 8
    assert pre64 + 216 * 48 == len(want)
    spots = [0, 31, rec0, rec0 + 1, rec0 + 1 + 128 + 8, rec0 + 1 + 128 + 8 + 5, pre2 - 8 - 1, pre2, pre2 + 15, pre2 + 16, pre2 + 47 + 48 * 100,
             pre2 + 216 * 48 + 8, pre64 - 8 - 1, pre64 + 3, len(want) - 1]
    rejected = 0
    for at in spots:
        data = bytearray(want)
        data[at] ^= 0x04
        for strict in (True, False):
            p0 = paths()
            dev = answer(rv, prog, wc, upload(data), strict)
            assert sum(delta(paths(), p0)) == 1
            host = answer(rv, prog, wc, bytes(data), strict)
            assert dev == host, (at, strict, dev, host)
            rejected += host is not True
    assert rejected >= 4  # (at the least the two flips inside comm, in both modes)
    # truncated proofs and a count of 41 take the fallback, with the host form's result
    for n in (1, 31, 40, pre2 + 5, len(want) - 1):
        assert both(rv, prog, wc, want[:n], True, 1) == (("error", E_MALFORMED),) * 2, n
    for which in ((0,), (1,), (0, 1)):
        d41 = proof_mutate._copy(doms)
        for d in which:
            d41[d] = (d41[d][0] + d41[d][0][-1:], d41[d][1])
        for strict in (True, False):
            assert both(rv, prog, wc, proof_mutate.serialise(comm, d41), strict, 1) == (False, False), which
    # a batch of three with the middle proof truncated: refused alone
    for trio in ([want, want[:len(want) - 9], want], [want, proof_mutate.serialise(comm, d41), want]):
        p0, t0 = paths(), traffic()
        oks = rv.verify_streaming_batch(prog, wc, [upload(p) for p in trio], max_chunk_ops=CHUNK)
        assert oks == [True, False, True] == rv.verify_streaming_batch(prog, wc, trio, max_chunk_ops=CHUNK)
        assert delta(paths(), p0) == [2, 1]
        assert delta(traffic(), t0)[3] == 2 * len(want)  # (the host batch's two good proofs; the device batch sent none up)
    with pytest.raises(TypeError):
        rv.verify_streaming_batch(prog, wc, [upload(want), want], max_chunk_ops=CHUNK)


# ---- 10. the streaming evaluator with device witnesses ----
def test_evaluator_device_witnesses(rv, rule_seeds):
    import torch

    import test_gpu_eval_stream as tes

    rng = np.random.default_rng(0xE7A)
    gname, gprog, gwc = tes.SHAPES[0]
    assert gname == "gf2"
    mprog, mw2, mw64, mwc = fd.mixed_three_pieces()
    planted, pwc = tes._planted_program({150: (2, 2), 41: (64, 1)})
    cases_ = [(gprog, gwc, *tes._wits(rng, 1, gprog)), (mprog, mwc, np.asarray([mw2], np.uint8), np.asarray([mw64], np.uint64)),
              (planted, pwc, *tes._planted_witness(rng, 5, [(b, k) for b in range(0, 5, 2) for k in (1, 2)]))]
    for prog, wc, w2, w64 in cases_:
        B = w2.shape[0]
        want = rv.evaluate_streaming(prog, w2 if B > 1 else w2[0], w64 if B > 1 else w64[0], wc, max_chunk_ops=CHUNK, values=True)
        wide2 = torch.full((B, w2.shape[1] + 5), 0xEE, dtype=torch.uint8, device="cuda")
        wide64 = torch.full((B, w64.shape[1] + 3), -1, dtype=torch.int64, device="cuda")
        wide2[:, :w2.shape[1]] = torch.from_numpy(w2).cuda()
        wide64[:, :w64.shape[1]] = torch.from_numpy(w64.view(np.int64).copy()).cuda()
        g, z = wide2[:, :w2.shape[1]], wide64[:, :w64.shape[1]]  # strided rows
        t0 = traffic()
        got = rv.evaluate_streaming(prog, g if B > 1 else g[0], z if B > 1 else z[0], wc, max_chunk_ops=CHUNK, values=True)
        tes.same(got, want)
        assert delta(traffic(), t0)[:2] == [0, B * (w2.shape[1] + 8 * w64.shape[1])]
        # two feeds, device ops, the witness columns each feed's Inputs consume
        d_prog = fd.on_device(prog)
        se = rv.StreamingEvaluator(wc, batch=B, max_chunk_ops=64)
        try:
            cut = len(prog) // 2
            n2, n64 = tes._inputs(prog[:cut])
            se.feed(d_prog[:cut], g[:, :n2], z[:, :n64])
            se.feed(prog[cut:], g[:, n2:], z[:, n64:])
            tes.same(se.finish(values=True), want)
        finally:
            se.close()
    assert want.n_failed[0] == 2 and want.first_failed_op[0] == 41  # (the planted program: its failures were seen)
    # errors: a short witness and a stride below n, sticky as the host feed's
    from reverie_amd import _lib

    se = rv.StreamingEvaluator(pwc, batch=5, max_chunk_ops=64)
    try:
        with pytest.raises(rv.ReverieError) as e:
            se.feed(planted, g[:, :15], z)
        assert e.value.code == E_WITNESS_SHORT
        with pytest.raises(rv.ReverieError) as e2:
            se.feed(planted, g, z)
        assert e2.value.code == E_WITNESS_SHORT
    finally:
        se.close()
    se = rv.StreamingEvaluator(pwc, batch=5, max_chunk_ops=64)
    try:
        bad = _lib.DevWitness(g.data_ptr(), 16, 15, z.data_ptr(), 8, z.stride(0))
        assert _L().rv_eval_stream_feed_wdev(se.handle, planted.ctypes.data_as(C.c_void_p), len(planted), 0, C.byref(bad)) == E_ARG
        with pytest.raises(rv.ReverieError) as e3:
            se.feed(planted, g, z)
        assert e3.value.code == E_ARG
    finally:
        se.close()
