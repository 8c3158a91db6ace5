"""Witness text on the GPU (rv_witness_parse_device, rv_witness_reader_*, rv_witness_write_device) against the host
definition: every text of witness_cases from host bytes and from a GPU tensor at every source and destination offset 0..16, with
the destination inside a poisoned buffer (a 16-byte store that crosses a tile's end shows there) and the source inside a buffer of
'1' bytes (a load outside the text shows in the count); count-only, a short capacity, marks; windows for every cut; the writer; and
proofs from a parsed text, a parsed batch and a text read in windows, byte for byte the proofs of the host-parsed witness."""
import ctypes as C

import numpy as np
import pytest

import witness_cases as wc

pytestmark = pytest.mark.gpu

POISON = 0xA5


@pytest.fixture(scope="module")
def rv():
    import reverie_amd

    return reverie_amd


@pytest.fixture(scope="module")
def env(rv):
    """(lib, context, torch, tile size, writer tile size)"""
    import torch

    from reverie_amd import _lib

    L = _lib.lib()
    out = (C.c_uint32 * 2)()
    assert L.rv_hook_witness_text_tiles(out) == 0
    return L, rv.Context.default(), torch, int(out[0]), int(out[1])


@pytest.fixture(scope="module")
def cases(env):
    """[(name, text, parse_witness' bits)], computed once"""
    from reverie_amd.witness import parse_witness

    return [(name, text, parse_witness(text)) for name, text in wc.texts(env[3])]


def gpu_text(torch, text, off):
    """the text at byte offset `off` of a GPU buffer that holds '1' everywhere else -> (buffer, address of the text)"""
    buf = torch.full((len(text) + 48,), ord("1"), dtype=torch.uint8, device="cuda")
    if len(text):
        buf[off:off + len(text)] = torch.frombuffer(bytearray(text), dtype=torch.uint8).cuda()
    torch.cuda.synchronize()
    return buf, buf.data_ptr() + off


def raw_parse(env, text, src_off, dst_off, cap, on_device, marks=None, count_only=False):
    """one rv_witness_parse_device call -> (code, count, the whole destination buffer on the host, bits_before)"""
    L, ctx, torch, _, _ = env
    keep = None
    if on_device:
        keep, p_text = gpu_text(torch, text, src_off)
    else:
        keep = np.frombuffer(b"1" * src_off + text + b"1", np.uint8)
        p_text = keep.ctypes.data + src_off
    dst = torch.full((max(cap, 0) + 64,), POISON, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    n = C.c_size_t(777)
    mk = np.asarray(marks if marks is not None else [], np.uint64)
    before = np.full(len(mk), 999, np.uint64)
    rc = L.rv_witness_parse_device(ctx.handle, C.c_void_p(p_text), C.c_size_t(len(text)), C.c_int(1 if on_device else 0),
                                   None if count_only else C.c_void_p(dst.data_ptr() + dst_off), C.c_size_t(cap), C.byref(n),
                                   C.c_void_p(mk.ctypes.data) if len(mk) else None, C.c_size_t(len(mk)), C.c_void_p(before.ctypes.data) if len(mk) else None)
    del keep
    return rc, n.value, dst.cpu().numpy(), before


def check_written(name, got, dst_off, want):
    n = len(want)
    assert (got[dst_off:dst_off + n] == want).all(), name
    assert (got[:dst_off] == POISON).all() and (got[dst_off + n:] == POISON).all(), name  # not one byte outside [0, n)


@pytest.mark.parametrize("on_device", [False, True], ids=["host-bytes", "gpu-tensor"])
def test_parse_equals_host_on_every_case(env, cases, on_device):
    """every case, with the source and destination offsets stepping through 0..16 (every value of both is met several times)"""
    for k, (name, text, want) in enumerate(cases):
        src_off, dst_off = k % 17, (5 * k + 3) % 17
        rc, n, got, _ = raw_parse(env, text, src_off, dst_off, len(want), on_device)  # exactly enough room
        assert (rc, n) == (0, len(want)), name
        check_written(name, got, dst_off, want)


def test_every_source_and_destination_offset(env, cases):
    """all 17 x 17 offsets for a text whose tiles end inside a 16-byte chunk of the destination, from a GPU tensor"""
    T = env[3]
    by_name = {name: (text, want) for name, text, want in cases}
    for name in (f"alternating-{2 * T + 1}", f"near-{T + 1}"):
        text, want = by_name[name]
        assert 0 < len(want) < len(text)
        for src_off in range(17):
            for dst_off in range(17):
                rc, n, got, _ = raw_parse(env, text, src_off, dst_off, len(want) + 5, True)
                assert (rc, n) == (0, len(want)), (name, src_off, dst_off)
                check_written((name, src_off, dst_off), got, dst_off, want)


def test_python_faces(env, cases):
    from reverie_amd import witness

    torch = env[2]
    for name, text, want in cases[::5]:
        for data in (text, np.frombuffer(text, np.uint8), torch.frombuffer(bytearray(text), dtype=torch.uint8).cuda() if text else torch.empty(0, dtype=torch.uint8, device="cuda")):
            got = witness.parse_device(data)
            assert got.device.type == "cuda" and got.dtype == torch.uint8 and (got.cpu().numpy() == want).all(), name


def test_count_only_and_short_capacity(env, cases):
    for k, (name, text, want) in enumerate(cases):
        on_device = bool(k & 1)
        rc, n, _, _ = raw_parse(env, text, k % 16, 0, 0, on_device, count_only=True)
        assert (rc, n) == (0, len(want)), name
        if len(want):  # one byte short, and no room at all: the count, and every destination byte as it was
            for cap in (len(want) - 1, 0):
                rc, n, got, _ = raw_parse(env, text, k % 16, (k * 3) % 17, cap, on_device)
                assert (rc, n) == (wc.ARG, len(want)) and (got == POISON).all(), (name, cap)


def test_marks(env, cases):
    """marks at 0, at len and one byte around every tile edge; the edges lie on aligned addresses, so they move with the source offset"""
    from reverie_amd.witness import parse_witness

    T = env[3]
    for k, (name, text, want) in enumerate(cases):
        if len(text) < T - 1 and k % 4:
            continue
        src_off = (7 * k) % 17
        marks = {0, len(text)}
        for edge in range(T, len(text) + T + 1, T):
            marks |= {p for p in (edge - (src_off % 16) + d for d in (-1, 0, 1)) if 0 <= p <= len(text)}
        marks = sorted(marks)
        for on_device in (True, False):
            rc, n, _, before = raw_parse(env, text, src_off, 0, len(want), on_device, marks=marks)
            assert (rc, n) == (0, len(want)), name
            assert before.tolist() == [len(parse_witness(text[:p])) for p in marks], (name, on_device)
    # marks are validated before anything runs: descending, or past the end
    name, text, want = cases[20]
    for bad in ([3, 2], [len(text) + 1]):
        assert raw_parse(env, text, 0, 0, len(want), False, marks=bad)[0] == wc.ARG


def test_arguments(env):
    L, ctx, torch, T, _ = env
    n = C.c_size_t()
    host = np.frombuffer(b"0101", np.uint8)
    dst = torch.zeros(64, dtype=torch.uint8, device="cuda")
    # a host pointer passed as device text or as d_bits, and a destination that overlaps a device text
    assert L.rv_witness_parse_device(ctx.handle, C.c_void_p(host.ctypes.data), 4, 1, C.c_void_p(dst.data_ptr()), 4, C.byref(n), None, 0, None) == wc.ARG
    assert L.rv_witness_parse_device(ctx.handle, C.c_void_p(host.ctypes.data), 4, 0, C.c_void_p(host.ctypes.data), 4, C.byref(n), None, 0, None) == wc.ARG
    assert L.rv_witness_parse_device(ctx.handle, C.c_void_p(dst.data_ptr()), 32, 1, C.c_void_p(dst.data_ptr() + 16), 32, C.byref(n), None, 0, None) == wc.ARG
    assert L.rv_witness_parse_device(ctx.handle, C.c_void_p(dst.data_ptr()), 32, 1, C.c_void_p(dst.data_ptr() + 32), 32, C.byref(n), None, 0, None) == 0
    assert L.rv_witness_parse_device(ctx.handle, C.c_void_p(host.ctypes.data), C.c_size_t(1 << 32), 0, None, 0, C.byref(n), None, 0, None) == wc.UNSUPPORTED
    assert L.rv_witness_parse_device(ctx.handle, None, 0, 0, None, 0, C.byref(n), None, 0, None) == 0 and n.value == 0  # the empty text


# ---- windows ----
def feed_all(witness, torch, text, cuts, flip=0):
    """the text fed in the pieces the cut points make, alternately from host bytes and from ranges of a GPU tensor -> (bits, totals)"""
    whole = torch.frombuffer(bytearray(text), dtype=torch.uint8).cuda() if text else torch.empty(0, dtype=torch.uint8, device="cuda")
    parts = []
    with witness.DeviceReader() as r:
        edges = [0] + list(cuts) + [len(text)]
        for i, (a, b) in enumerate(zip(edges, edges[1:])):
            parts.append(r.feed(whole[a:b] if (i + flip) & 1 else text[a:b]))
        totals = r.finish()
    return torch.cat(parts).cpu().numpy(), totals


def test_windows_every_two_way_cut_of_the_short_texts(env):
    from reverie_amd import witness

    torch, T = env[2], env[3]
    tried = 0
    for name, text in wc.short_texts(T):
        want = witness.parse_witness(text)
        for cut in range(len(text) + 1):
            got, totals = feed_all(witness, torch, text, [cut], flip=cut)
            assert (got == want).all() and len(got) == len(want) and totals == (len(text), len(want)), (name, cut)
            tried += 1
    assert tried > 500


def test_windows_seeded_cuts_of_the_tile_edge_texts(env):
    from reverie_amd import witness

    torch, T = env[2], env[3]
    texts = wc.edge_texts(T)
    rng = np.random.default_rng(50)
    for k in range(50):
        name, text = texts[k % len(texts)] if k < len(texts) else texts[int(rng.integers(len(texts)))]
        near = [e + d for e in range(T, len(text) + 1, T) for d in (-1, 0, 1) if 0 <= e + d <= len(text)]
        cuts = sorted({int(rng.integers(0, len(text) + 1)) for _ in range(int(rng.integers(1, 4)))} | ({int(rng.choice(near))} if near else set()))
        got, totals = feed_all(witness, torch, text, cuts, flip=k)
        want = witness.parse_witness(text)
        assert len(got) == len(want) and (got == want).all() and totals == (len(text), len(want)), (name, cuts)


def test_windows_tiny_feeds_and_a_refused_feed(env):
    from reverie_amd import witness

    L, ctx, torch, T, _ = env
    text = b"01x1\r\n0/2" + bytes([0xB0, 0xB1, 0]) + b"1100 1"
    want = witness.parse_witness(text)
    parts = []
    with witness.DeviceReader() as r:
        for i in range(len(text)):  # feeds of length 1, with feeds of length 0 between them
            parts.append(r.feed(text[i:i + 1]))
            assert r.feed(b"").numel() == 0
        assert r.finish() == (len(text), len(want))
    assert torch.cat(parts).cpu().numpy().tolist() == want.tolist()
    # a feed refused for its capacity leaves the reader as it was; the same bytes are fed again
    big = (b"01" * 40 + b"\n") * 60
    wbig = witness.parse_witness(big)
    h = C.c_void_p()
    assert L.rv_witness_reader_begin(ctx.handle, C.byref(h)) == 0
    try:
        n, a, b = C.c_size_t(), C.c_uint64(), C.c_uint64()
        first = np.frombuffer(big[:1000], np.uint8)
        dst = torch.full((8192,), POISON, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        assert L.rv_witness_reader_feed(h, C.c_void_p(first.ctypes.data), 1000, 0, C.c_void_p(dst.data_ptr()), 4096, C.byref(n)) == 0
        n_first = n.value
        rest = np.frombuffer(big[1000:], np.uint8)
        assert L.rv_witness_reader_feed(h, C.c_void_p(rest.ctypes.data), len(rest), 0, C.c_void_p(dst.data_ptr() + 4096), 100, C.byref(n)) == wc.ARG
        assert n.value == len(wbig) - n_first
        assert L.rv_witness_reader_finish(h, C.byref(a), C.byref(b)) == 0 and (a.value, b.value) == (1000, n_first)  # unchanged
        assert (dst[4096:].cpu().numpy() == POISON).all()  # and nothing written
        assert L.rv_witness_reader_feed(h, C.c_void_p(rest.ctypes.data), len(rest), 0, C.c_void_p(dst.data_ptr() + 4096), 4096, C.byref(n)) == 0
        assert L.rv_witness_reader_finish(h, C.byref(a), C.byref(b)) == 0 and (a.value, b.value) == (len(big), len(wbig))
        got = dst.cpu().numpy()
        assert (np.concatenate([got[:n_first], got[4096:4096 + n.value]]) == wbig).all()
    finally:
        L.rv_witness_reader_destroy(h)
    # the Python face grows a buffer that is too small
    with witness.DeviceReader() as r:
        out = torch.empty(10, dtype=torch.uint8, device="cuda")
        assert (r.feed(big, out=out).cpu().numpy() == wbig).all() and r.finish() == (len(big), len(wbig))


# ---- the writer ----
def raw_write(env, bits, line_bits, off, room):
    L, ctx, torch, _, _ = env
    d_bits = torch.from_numpy(np.ascontiguousarray(bits)).cuda() if len(bits) else None
    dst = torch.full((room + 64,), POISON, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    n = C.c_size_t(777)
    rc = L.rv_witness_write_device(ctx.handle, C.c_void_p(d_bits.data_ptr()) if d_bits is not None else None, C.c_size_t(len(bits)), C.c_uint64(line_bits),
                                   C.c_void_p(dst.data_ptr() + off), C.c_size_t(room), C.byref(n))
    return rc, n.value, dst.cpu().numpy()


def test_writer_equals_host(env):
    from reverie_amd import witness

    torch, T = env[2], env[3]
    rng = np.random.default_rng(9)
    k = 0
    for n in (0, 1, 15, 16, 17, T - 1, T, T + 1, 2 * T - 1, 2 * T, 2 * T + 1):
        bits = rng.integers(0, 2, n, dtype=np.uint8)
        for lb in wc.line_bits_values(n):
            want = witness.dumps(bits, lb)
            off = k % 17  # (a misaligned d_text: every offset is met)
            k += 1
            rc, length, got = raw_write(env, bits, lb, off, len(want))  # exactly enough room
            assert (rc, length) == (0, len(want)), (n, lb)
            assert got[off:off + length].tobytes() == want and (got[:off] == POISON).all() and (got[off + length:] == POISON).all(), (n, lb, off)
            if want:
                rc, length, got = raw_write(env, bits, lb, off, len(want) - 1)  # too small: the length, nothing written
                assert (rc, length) == (wc.ARG, len(want)) and (got == POISON).all(), (n, lb)
        if n:
            text = witness.dumps_device(torch.from_numpy(bits).cuda(), 64)
            assert text.device.type == "cuda" and bytes(text.cpu().numpy()) == witness.dumps(bits, 64)
            assert (witness.parse_device(text).cpu().numpy() == bits).all()  # and back, without leaving the GPU
    assert witness.dumps_device(torch.empty(0, dtype=torch.uint8, device="cuda")).numel() == 0


def test_writer_refuses_a_byte_above_one(env):
    T = env[3]
    n = 3 * T + 5  # four tiles of output at 64 bits a line
    for at in (0, 1, n - 1, n - 2, T + 7, None):
        bits = np.zeros(n, np.uint8)
        if at is not None:
            bits[at] = 2
        rc, length, _ = raw_write(env, bits, 64, 3, 2 * n)
        assert rc == (wc.ARG if at is not None else 0) and length == n + -(-n // 64), at


# ---- end to end: proofs from a parsed text are the proofs of the host-parsed witness ----
@pytest.fixture(scope="module")
def aes(rv):
    """(circuit, ops, wire counts, three witness texts with their host-parsed bits, seeds [3][256][16])"""
    import bristol_gen
    from reverie_amd import bristol, witness

    prog, info = bristol.parse(bristol_gen.aes128())
    wcnt = info["wire_counts"]
    rng = np.random.default_rng(128)
    texts = []
    for b in range(3):
        bits = rng.integers(0, 2, 256, dtype=np.uint8)
        text = b"# key and block " + b"abc"[b:b + 1] + b"\r\n" + witness.dumps(bits, 64).replace(b"\n", b" /2\r\n")
        texts.append((text, witness.parse_witness(text)))
        assert (texts[-1][1] == bits).all()
    seeds = rng.integers(0, 256, (3, 256, 16), dtype=np.uint8)
    return rv.Circuit(prog, wcnt), prog, wcnt, texts, seeds


def traffic(L):
    out = (C.c_uint64 * 3)()
    assert L.rv_hook_witness_traffic(out) == 0
    return tuple(int(x) for x in out)


def test_proof_from_a_parsed_text(rv, env, aes):
    from reverie_amd import witness

    L, _, torch, _, _ = env
    c, _, _, texts, seeds = aes
    text, bits = texts[0]
    want = bytes(rv.Proof.new(c, bits, [], seeds=seeds[0]))
    assert bytes(rv.Proof.new(c, witness.parse_device(text), [], seeds=seeds[0])) == want
    # with the text in a GPU tensor no witness byte goes host-to-device; from host bytes the text's bytes do, and nothing else
    d_text = torch.frombuffer(bytearray(text), dtype=torch.uint8).cuda()
    before = traffic(L)
    assert bytes(rv.Proof.new(c, witness.parse_device(d_text), [], seeds=seeds[0])) == want
    after = traffic(L)
    assert after[0] == before[0] and after[1] > before[1]
    witness.parse_device(text)
    assert traffic(L)[0] == after[0] + len(text)


def test_proofs_from_a_parsed_batch(rv, env, aes):
    from reverie_amd import witness

    torch = env[2]
    c, _, _, texts, seeds = aes
    want = [bytes(rv.Proof.new(c, bits, [], seeds=seeds[b])) for b, (_, bits) in enumerate(texts)]
    wits = witness.parse_device_batch([t for t, _ in texts])
    assert tuple(wits.shape) == (3, 256) and (wits.cpu().numpy() == np.stack([b for _, b in texts])).all()
    assert [bytes(p) for p in rv.Proof.new_batch(c, wits, seeds=seeds)] == want
    # texts that lie in GPU memory, and one that does not: the same rows
    mixed = [torch.frombuffer(bytearray(texts[0][0]), dtype=torch.uint8).cuda(), texts[1][0], np.frombuffer(texts[2][0], np.uint8)]
    assert (witness.parse_device_batch(mixed).cpu().numpy() == wits.cpu().numpy()).all()
    with pytest.raises(ValueError, match="text 2 holds 255 bits"):
        witness.parse_device_batch([texts[0][0], texts[1][0], texts[2][0][:-6] + b"\r\n"])


def aes_pieces(prog):
    cuts = [0, 100, 300, 9000, len(prog)]  # (the 256 Input ops lead: the first two pieces share them)
    return lambda: iter([(prog[a:b], None) for a, b in zip(cuts, cuts[1:])])


def test_streamed_proof_from_a_text_in_windows(rv, env, aes):
    from reverie_amd import stream, witness

    torch = env[2]
    _, prog, wcnt, texts, seeds = aes
    text, bits = texts[1]
    want, _ = stream.prove_streaming(prog, bits, [], wcnt, seeds=seeds[1])
    for source in (text, torch.frombuffer(bytearray(text), dtype=torch.uint8).cuda()):
        with witness.DeviceWindows(source, window_bytes=64) as w:
            got, _ = stream.prove_streaming_pieces(aes_pieces(prog), w, [], wcnt, seeds=seeds[1])
        assert bytes(got) == bytes(want)
    with witness.DeviceWindows(text, window_bytes=64) as w:
        r = stream.evaluate_streaming_pieces(aes_pieces(prog), w, [], wcnt)
    assert bool(r.ok[0])
    # take by take: the bits in order, across windows, and from the start again after a rewind
    with witness.DeviceWindows(text, window_bytes=7) as w:
        assert w.take(0).numel() == 0 and w.take(100).cpu().numpy().tolist() == bits[:100].tolist()
        assert w.take(156).cpu().numpy().tolist() == bits[100:].tolist()
        w.rewind()
        assert w.take(256).cpu().numpy().tolist() == bits.tolist()


def test_a_text_one_bit_short(rv, env, aes):
    from reverie_amd import stream, witness

    c, prog, wcnt, texts, seeds = aes
    short = [t[:t.rindex(b"1" if b[-1] else b"0")] + b"\r\n" for t, b in texts]  # the last bit cut off
    assert [len(witness.parse_witness(t)) for t in short] == [255] * 3
    with pytest.raises(rv.ReverieError) as e:
        rv.Proof.new(c, witness.parse_device(short[0]), [], seeds=seeds[0])
    assert e.value.code == wc.WITNESS_SHORT
    with pytest.raises(rv.ReverieError) as e:
        rv.Proof.new_batch(c, witness.parse_device_batch(short), seeds=seeds)
    assert e.value.code == wc.WITNESS_SHORT
    with pytest.raises(rv.ReverieError) as e:
        with witness.DeviceWindows(short[1], window_bytes=64) as w:
            stream.prove_streaming_pieces(aes_pieces(prog), w, [], wcnt, seeds=seeds[1])
    assert e.value.code == wc.WITNESS_SHORT
