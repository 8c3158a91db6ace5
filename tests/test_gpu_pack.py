"""The kernels that turn transcript rows into proof vectors and back -- k_extract_rows<0|1>, k_extract_from_bits, k_pack_corr_all,
k_copy_gaps, k_unpack_bits (open.hip), k_extract64, k_extract64_ol, k_unpack64 (z64.hip) -- one production launch at a time against
tests/pack_ref.py, byte for byte: at vector lengths of every residue mod 8 and on the tile edges, at every tile ex_tb_for can pick,
at row widths that take each kernel's other loop, under opening maps a hash output does not produce, and at every source alignment.

The rv_hook_* entry points call the production launch_* functions unchanged and return every output buffer whole; outputs start as
0xA5, and a byte outside the expected vectors must still be 0xA5 afterwards (records lie side by side in a proof: a one-byte overrun
is a wrong proof).  tests/test_pack_ref_host.py ties the reference to the CPU oracle.

Not tested: more than 40 opened repetitions (ex_slots clamps there, production never exceeds it and the hooks refuse it).
k_fs_challenge, k_open_headers, k_open_small and k_frame_counts have their own file, tests/test_gpu_open_heads.py (which leaves out the
second draw round of k_fs_challenge: no input is known that needs one)."""
import ctypes as C
import functools

import numpy as np
import pytest

import pack_ref

pytestmark = pytest.mark.gpu

FILL = 0xA5
FILL32 = 0xA5A5A5A5
FILL64 = 0xA5A5A5A5A5A5A5A5
E_ARG = 9
WIDTHS = [8, 24, 32, 64, 88, 256]  # NQ = 2, 6, 8, 16, 22, 64: NQ = 6 and 22 take k_unpack_bits' plain loop, NQ = 6 the byte loop of k_extract_from_bits
LENGTHS = [0, 1, 7, 8, 9, 55, 56, 63, 64, 65]  # one, two and (with the window sizes below) many workgroups at tile 8
WINDOW = 8 * 64  # items of one UNP_TB window of k_unpack_bits / of one workgroup of k_pack_corr_all
UNPACK_LENGTHS = LENGTHS + [WINDOW - 8, WINDOW - 1, WINDOW, WINDOW + 1, WINDOW + 8]
TILES_ROWS = [16, 32, 64, 128, 256]
TILES_BITS = [16, 32, 64, 128]
MIN_GROUPS = 2048  # ex_tb_for halves the tile until there are this many workgroups


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _u64(v):
    return np.ascontiguousarray(np.asarray(v, np.uint64))


@pytest.fixture(scope="module")
def hooks():
    import reverie_amd
    from reverie_amd import _lib

    ctx = reverie_amd.Context.default()  # raises loudly if the HIP library or the GPU is missing
    return _lib.lib(), ctx.handle


def tile_length(tile, cap, residue):
    """the shortest vector that ex_tb_for gives `tile` bytes per workgroup (cap = the kernel's largest), n_items % 8 = residue:
    the tile is halved while ceil(n_bytes / tile) < 2048, so tile T needs n_bytes > 2047 T -- and one byte less takes T / 2"""
    assert 8 < tile <= cap
    n_b = (MIN_GROUPS - 1) * tile + 1
    n = 8 * (n_b - 1) + residue
    assert pack_ref.n_bytes(n) == n_b
    return n


# ---- opening maps (fixed seeds) ----
def _with_players(reps, R, seed):
    """omit[R]: the listed repetitions opened, players from a fixed seed with every player 0..7 present when there is room"""
    rng = np.random.default_rng(seed)
    omit = np.full(R, 8, np.uint8)
    reps = np.asarray(reps, np.int64)
    pl = rng.integers(0, 8, len(reps))
    if len(reps) >= 8:
        pl[:8] = rng.permutation(8)
    omit[reps] = pl
    return omit


@functools.lru_cache(maxsize=None)
def maps(R):
    """{name: omit[R]} -- at most 40 opened"""
    rng = np.random.default_rng(500 + R)
    k = min(40, R // 2)
    out = {
        "scattered": _with_players(np.sort(rng.permutation(R)[:k]), R, 1),  # R = 256: production-like, 40 with every player
        "first": _with_players(np.arange(min(40, R)), R, 2),                # the verifier's slot order
        "last": _with_players(np.arange(R - min(40, R), R), R, 3),
        "one@0": _with_players([0], R, 4),
        "one@end": _with_players([R - 1], R, 5),
        "none": np.full(R, 8, np.uint8),
    }
    if R >= 64:
        quads = np.sort(rng.permutation(R // 4)[:10])
        out["tenquads"] = _with_players((4 * quads[:, None] + np.arange(4)).reshape(-1), R, 6)
    if R == 256:
        assert set(out["scattered"][out["scattered"] < 8].tolist()) == set(range(8)) and (out["scattered"] < 8).sum() == 40
    for v in out.values():
        v.setflags(write=False)
    return out


def layout(omit, length, seed, base=5, tail=9):
    """vectors of `length` bytes side by side in a shuffled order from an odd offset: dst_off[R] and the buffer's size"""
    on = pack_ref.opened(omit)
    order = np.random.default_rng(seed).permutation(len(on))
    at = np.zeros(len(omit), np.uint64)
    for slot, k in enumerate(order):
        at[on[k]] = base + slot * length
    return at, base + len(on) * length + tail


def check_bytes(got, vecs, at, what):
    want, spans = pack_ref.image(FILL, len(got), vecs, at)
    if not np.array_equal(got, want):
        pytest.fail(f"{what}: first wrong byte: {pack_ref.first_diff_bytes(got, want, spans)}")


# ---- k_extract_rows ----
def call_extract_bits(hooks, stream, rows, n, R, kind, omit, at, out, out2=None, n_direct=0, gaps=None):
    L, h = hooks
    tile = C.c_uint32(0)
    stream = np.ascontiguousarray(stream, np.uint32)
    rc = L.rv_hook_extract_bits(h, _p(stream), stream.shape[0], _p(rows), n, R, kind, _p(omit), _p(at), _p(out), len(out), _p(out2), n_direct,
                                _p(gaps), C.byref(tile))
    return rc, tile.value


def _row_stream(R, kind, n_rows, seed):
    rng = np.random.default_rng(seed)
    if kind == 0:
        return rng.integers(0, 2**32, (n_rows, R // 4), dtype=np.uint64).astype(np.uint32)
    return pack_ref.recon_rows_from_items(rng.integers(0, 2, (n_rows, R), dtype=np.uint8))


@pytest.mark.parametrize("kind", [0, 1])
@pytest.mark.parametrize("R", WIDTHS)
def test_extract_rows(hooks, R, kind):
    pool = _row_stream(R, kind, 97, 10 * R + kind)
    rng = np.random.default_rng(R + kind)
    for name, omit in maps(R).items():
        for n in LENGTHS + [WINDOW - 1, 8 * 8 * 3]:
            for listed in (False, True):
                ids = rng.integers(0, len(pool), n).astype(np.uint32) if listed else None
                stream = pool if listed else np.ascontiguousarray(pool[rng.integers(0, len(pool), n)])
                vecs = pack_ref.pack_rows(stream, omit, kind, ids)
                at, size = layout(omit, pack_ref.n_bytes(n), n)
                out = np.full(size, FILL, np.uint8)
                rc, tile = call_extract_bits(hooks, stream, ids, n, R, kind, omit, at, out)
                what = f"k_extract_rows<{kind}>, R = {R}, map {name}, n_items = {n}, {'row list' if listed else 'rows in order'}, tile {tile}"
                assert rc == 0, f"{what}: error {rc}"
                assert tile == 8, what
                check_bytes(out, vecs, at, what)


@pytest.mark.parametrize("kind", [0, 1])
@pytest.mark.parametrize("tile", TILES_ROWS)
def test_extract_rows_tiles(hooks, tile, kind):
    """one long vector per larger tile, at the shortest length that takes it, n_items % 8 zero and not"""
    R = 32
    omit = _with_players([0, 5, 6, 12, 13, 14, 15, 31], R, 7)  # a quad with one, two, four and none opened; both ends
    pool = _row_stream(R, kind, 4099, 20 + kind)
    for residue in (0, 3):
        n = tile_length(tile, 256, residue)
        ids = np.random.default_rng(tile + residue).integers(0, len(pool), n).astype(np.uint32)
        vecs = pack_ref.pack_rows(pool, omit, kind, ids)
        at, size = layout(omit, pack_ref.n_bytes(n), tile)
        out = np.full(size, FILL, np.uint8)
        rc, got_tile = call_extract_bits(hooks, pool, ids, n, R, kind, omit, at, out)
        what = f"k_extract_rows<{kind}>, R = {R}, n_items = {n}, tile {got_tile}"
        assert rc == 0, f"{what}: error {rc}"
        assert got_tile == tile, f"{what}: expected tile {tile}"
        check_bytes(out, vecs, at, what)


def test_extract_rows_all_opened(hooks):
    """R = 32 with all 32 opened: the shard has no preprocessing record"""
    R = 32
    omit = _with_players(np.arange(R), R, 8)
    for kind in (0, 1):
        stream = _row_stream(R, kind, 70, 30 + kind)
        for n in (0, 9, 64, 70):
            vecs = pack_ref.pack_rows(stream[:n], omit, kind)
            at, size = layout(omit, pack_ref.n_bytes(n), n)
            out = np.full(size, FILL, np.uint8)
            rc, tile = call_extract_bits(hooks, stream, None, n, R, kind, omit, at, out)
            assert rc == 0
            check_bytes(out, vecs, at, f"k_extract_rows<{kind}>, R = 32 all opened, n_items = {n}")


# ---- k_extract_from_bits ----
def call_extract_from_bits(hooks, bits, n, R, omit, at, rep_min, out):
    L, h = hooks
    tile = C.c_uint32(0)
    rc = L.rv_hook_extract_from_bits(h, _p(bits), n, R, _p(omit), _p(at), rep_min, _p(out), len(out), C.byref(tile))
    return rc, tile.value


def _check_from_bits(hooks, bits, n, R, omit, rep_min, want_tile, what):
    reps = [r for r in pack_ref.opened(omit) if r >= rep_min]
    vecs = pack_ref.pack_bitstream(bits[:n], reps)
    at, size = layout(omit, pack_ref.n_bytes(n), n + rep_min)
    out = np.full(size, FILL, np.uint8)
    rc, tile = call_extract_from_bits(hooks, bits, n, R, omit, at, rep_min, out)
    what = f"k_extract_from_bits, {what}, n_items = {n}, rep_min = {rep_min}, tile {tile}"
    assert rc == 0, f"{what}: error {rc}"
    assert tile == want_tile, f"{what}: expected tile {want_tile}"
    check_bytes(out, vecs, at, what)


@pytest.mark.parametrize("R", WIDTHS)
def test_extract_from_bits(hooks, R):
    bits = np.random.default_rng(40 + R).integers(0, 256, (WINDOW + 8, R // 8), dtype=np.uint8)
    all_opened = {"all": _with_players(np.arange(R), R, 8)} if R == 32 else {}
    for name, omit in {**maps(R), **all_opened}.items():
        for n in LENGTHS + [WINDOW - 1, WINDOW + 1]:
            for rep_min in (0, R // 2, R):
                _check_from_bits(hooks, bits, n, R, omit, rep_min, 8, f"R = {R}, map {name}")


@pytest.mark.parametrize("tile", TILES_BITS)
def test_extract_from_bits_tiles(hooks, tile):
    R = 32
    omit = _with_players([0, 5, 6, 12, 13, 14, 15, 31], R, 7)
    n_max = tile_length(tile, 128, 3)
    bits = np.random.default_rng(50 + tile).integers(0, 256, (n_max, R // 8), dtype=np.uint8)
    for residue in (0, 3):
        _check_from_bits(hooks, bits, tile_length(tile, 128, residue), R, omit, 0, tile, f"R = {R}")


# ---- k_pack_corr_all, and the cross-check with k_extract_from_bits ----
@functools.lru_cache(maxsize=None)
def _corr_case(n):
    bits = np.random.default_rng(60 + n).integers(0, 256, (n, 32), dtype=np.uint8)
    vecs = pack_ref.pack_bitstream(bits, range(256))
    full = np.stack([vecs[r] for r in range(256)])  # [256, n // 8 + 1]
    full.setflags(write=False)
    return bits, full


PACK_CORR_LENGTHS = LENGTHS + [k * WINDOW + d for k in (1, 2, 3) for d in (-1, 0, 1)]


@pytest.mark.parametrize("n", PACK_CORR_LENGTHS)
def test_pack_corr_all(hooks, n):
    L, h = hooks
    bits, full = _corr_case(n)
    nb = pack_ref.n_bytes(n)
    # (byte0, n_bytes): the whole vector; from a later byte; a length that is no multiple of 16; a chunk that runs past the vector's end
    # (zeros there) and one wholly past the last item
    chunks = [(0, nb), (0, nb + 20), (nb + 3, 37)]
    if nb > 1:
        chunks += [(1, nb - 1), (nb // 2, nb - nb // 2 + 5)]
    if nb > 64:
        chunks += [(64, nb - 64), (64, 21), (3, 64)]
    omit = maps(256)["scattered"]
    for byte0, n_b in chunks:
        pitch = 128 * ((n_b + 127) // 128)
        want = np.zeros((256, n_b), np.uint8)
        have = full[:, byte0:byte0 + n_b]
        want[:, :have.shape[1]] = have
        out = np.full((256, pitch), FILL, np.uint8)
        rc = L.rv_hook_pack_corr_all(h, _p(bits), n, byte0, n_b, pitch, _p(out))
        what = f"k_pack_corr_all, n_items = {n}, byte0 = {byte0}, n_bytes = {n_b}, pitch = {pitch}"
        assert rc == 0, f"{what}: error {rc}"
        if not np.array_equal(out[:, :n_b], want):
            r, b = (int(x) for x in np.argwhere(out[:, :n_b] != want)[0])
            pytest.fail(f"{what}: first wrong byte: repetition {r}, byte {byte0 + b} of the vector (chunk byte {b}): got 0x{out[r, b]:02x}, "
                        f"want 0x{want[r, b]:02x}")
        pad = 16 * ((n_b + 15) // 16)  # (whole 16-byte words: the bytes up to there are padding)
        assert (out[:, pad:] == FILL).all(), f"{what}: bytes past the chunk's last 16-byte word were written"
        # the opened repetitions' vectors from k_extract_from_bits, over the same range
        at, size = layout(omit, nb, n)
        ex = np.full(size, FILL, np.uint8)
        rc, _ = call_extract_from_bits(hooks, bits, n, 256, omit, at, 0, ex)
        assert rc == 0
        for r in pack_ref.opened(omit):
            vec = np.zeros(byte0 + n_b, np.uint8)
            vec[:min(nb, byte0 + n_b)] = ex[int(at[r]):int(at[r]) + nb][:byte0 + n_b]
            assert np.array_equal(out[r, :n_b], vec[byte0:]), f"{what}: repetition {r} differs from k_extract_from_bits' vector"


# ---- k_unpack_bits ----
def call_unpack_bits(hooks, blob, off, ln, omit, n, R, kind, out_nq, first_item, rows):
    L, h = hooks
    return L.rv_hook_unpack_bits(h, _p(blob), len(blob), _p(off), _p(ln), _p(omit), n, R, kind, out_nq, first_item, _p(rows))


def _src_lengths(n_total_bytes, k):
    """the forms of src_len, dealt over the opened repetitions: exact, longer, 0, 1, ending inside a window, ending on a window edge"""
    form = k % 6
    if form == 0:
        return n_total_bytes
    if form == 1:
        return n_total_bytes + 7
    if form == 2:
        return 0
    if form == 3:
        return 1
    if form == 4:
        return max(0, n_total_bytes - 3) if n_total_bytes < 64 else 64 * (n_total_bytes // 64) - 29
    return 64 * (n_total_bytes // 64) if n_total_bytes >= 64 else n_total_bytes


def _check_unpack_bits(hooks, R, kind, omit, n, first_item, out_nq, forms, seed, what):
    """vectors of (first_item + n) items at every alignment mod 4 in a blob of noise, src_len in every form"""
    rng = np.random.default_rng(seed)
    on = pack_ref.opened(omit)
    nb = pack_ref.n_bytes(first_item + n)
    blob = rng.integers(0, 256, 16 + len(on) * (nb + 12) + 16, dtype=np.uint8)
    off, ln = np.zeros(R, np.uint64), np.zeros(R, np.uint64)
    vecs, at = {}, 13
    for k, r in enumerate(on):
        at += (k + (seed % 4) - at) % 4  # start address = k + seed mod 4
        off[r] = at
        ln[r] = _src_lengths(nb, k) if forms else nb
        vecs[r] = blob[at:at + int(ln[r])]
        at += nb + 8
    assert at <= len(blob)
    want = pack_ref.unpack_rows(vecs, omit, n, R // 4, kind, first_item)[:, :out_nq]
    rows = np.full((n, out_nq), FILL32, np.uint32)
    rc = call_unpack_bits(hooks, blob, off, ln, omit, n, R, kind, out_nq, first_item, rows)
    path = "quad-compacted path" if 256 % (R // 4) == 0 else "plain loop"
    what = f"k_unpack_bits ({path}), kind {kind}, R = {R}, {what}, n_items = {n}, first_item = {first_item}, out_nq = {out_nq}"
    assert rc == 0, f"{what}: error {rc}"
    held = np.zeros(out_nq, bool)
    held[np.array([r // 4 for r in on if r // 4 < out_nq], np.int64)] = True
    if not np.array_equal(rows[:, held], want[:, held]):
        g, w = rows.copy(), want.copy()
        g[:, ~held] = 0
        w[:, ~held] = 0
        pytest.fail(f"{what}: first wrong word: {pack_ref.first_diff_rows(g, w)}")
    rest = rows[:, ~held]
    bad = np.argwhere((rest != 0) & (rest != FILL32))
    assert not len(bad), f"{what}: a quad word without an opened repetition is neither zero nor untouched: item {bad[0][0]}"


@pytest.mark.parametrize("kind", [0, 1])
@pytest.mark.parametrize("R", WIDTHS)
def test_unpack_bits(hooks, R, kind):
    all_opened = {"all": _with_players(np.arange(R), R, 8)} if R == 32 else {}
    for name, omit in {**maps(R), **all_opened}.items():
        for i, n in enumerate(UNPACK_LENGTHS):
            if n == 0:
                continue  # (launch_unpack_bits returns at once; checked below)
            _check_unpack_bits(hooks, R, kind, omit, n, 0, R // 4, False, 70 + i, f"map {name}, src_len exact")
            _check_unpack_bits(hooks, R, kind, omit, n, 0, R // 4, True, 80 + i, f"map {name}, src_len in every form")
    rows = np.full((4, R // 4), FILL32, np.uint32)
    omit = maps(R)["scattered"]
    z = np.zeros(R, np.uint64)
    assert call_unpack_bits(hooks, np.zeros(8, np.uint8), z, z, omit, 0, R, kind, R // 4, 0, rows) == 0 and (rows == FILL32).all()


@pytest.mark.parametrize("kind", [0, 1])
@pytest.mark.parametrize("R", [24, 64, 256])
def test_unpack_bits_first_item(hooks, R, kind):
    """the streaming verifier's offsets: every bit offset, a start in the second and in a later window"""
    omit = maps(R)["first"]
    firsts = list(range(8)) + [WINDOW + 3, WINDOW - 1, 5 * WINDOW + 5, 3 * WINDOW]
    for i, first in enumerate(firsts):
        for n in (1, 9, 64, WINDOW - 1, WINDOW + 8, 2 * WINDOW + 3):
            _check_unpack_bits(hooks, R, kind, omit, n, first, R // 4, i % 2 == 1, 90 + i, "map first")


@pytest.mark.parametrize("kind", [0, 1])
@pytest.mark.parametrize("R", [88, 256])
def test_unpack_bits_sixteen_quads(hooks, R, kind):
    """the verifier's slot order: all 40 in repetitions 0 .. 39, rows of sixteen quad words -- and the same at the full width"""
    omit = maps(R)["first"]
    for i, n in enumerate(UNPACK_LENGTHS[1:]):
        for out_nq in (16, R // 4):
            _check_unpack_bits(hooks, R, kind, omit, n, i % 8, out_nq, i % 2 == 0, 110 + i, "map first")


# ---- k_extract64, k_extract64_ol, k_unpack64 ----
Z64_VALUES = [0, 2**64 - 1, 1 << 63, 0x0102030405060708]


def _z64_stream(R, stride, seed):
    s = np.random.default_rng(seed).integers(0, 2**63, (R, stride), dtype=np.uint64) * np.uint64(2) + np.uint64(1)
    s[:, 0:4] = np.array(Z64_VALUES, np.uint64)
    s[:, 9:13] = np.array(Z64_VALUES, np.uint64)
    return s


@pytest.mark.parametrize("use_list", [0, 1], ids=["k_extract64", "k_extract64_ol"])
@pytest.mark.parametrize("R", [8, 64, 256])
def test_extract64(hooks, R, use_list):
    L, h = hooks
    stride = 140
    stream = _z64_stream(R, stride, 120 + R)
    rng = np.random.default_rng(R)
    for name, omit in maps(R).items():
        for n in [0, 1, 7, 8, 9, 31, 32, 33, 100]:
            for add_omit, listed in ((0, False), (1, False), (0, True), (1, True)):
                offs = _u64(rng.integers(0, stride - 8, n)) if listed else None
                for rep_min in ((0, R // 2, R) if use_list else (0,)):
                    vecs = {}
                    for r in pack_ref.opened(omit):
                        if use_list and r < rep_min:
                            continue
                        idx = (np.arange(n) if offs is None else offs.astype(np.int64)) + (int(omit[r]) if add_omit else 0)
                        vecs[r] = pack_ref.pack64(stream[r, idx])
                    at, size = layout(omit, 8 * n, n + add_omit, base=3, tail=11)
                    out = np.full(size, FILL, np.uint8)
                    rc = L.rv_hook_extract64(h, _p(stream), stride, _p(offs), n, add_omit, R, _p(omit), _p(at), use_list, rep_min, _p(out), len(out))
                    what = (f"{'k_extract64_ol' if use_list else 'k_extract64'}, R = {R}, map {name}, n_items = {n}, add_omit = {add_omit}, "
                            f"{'offset list' if listed else 'no offset list'}, stride {stride}, rep_min = {rep_min}")
                    assert rc == 0, f"{what}: error {rc}"
                    check_bytes(out, vecs, at, what)


@pytest.mark.parametrize("R", [8, 64, 256])
def test_unpack64(hooks, R):
    L, h = hooks
    rng = np.random.default_rng(130 + R)
    for name, omit in maps(R).items():
        on = pack_ref.opened(omit)
        for n in [1, 2, 7, 31, 32, 33, 100]:
            values = rng.integers(0, 2**63, (R, n), dtype=np.uint64) * np.uint64(2) + np.uint64(1)
            values[:, :min(n, 4)] = np.array(Z64_VALUES, np.uint64)[:min(n, 4)]
            blob = rng.integers(0, 256, 16 + len(on) * (8 * n + 24), dtype=np.uint8)
            off, ln = np.zeros(R, np.uint64), np.zeros(R, np.uint64)
            at = 5
            for k, r in enumerate(on):
                at += k % 3  # (any byte alignment)
                # src_len: exact, longer, 0, 1, no multiple of 8 (the partial item reads as zero), one item short
                ln[r] = [8 * n, 8 * n + 5, 0, 1, max(0, 8 * n - 3), 8 * (n - 1)][k % 6]
                off[r] = at
                blob[at:at + 8 * n] = pack_ref.pack64(values[r])
                at += 8 * n + 8
            outs = [R] + ([64] if R > 64 and name in ("first", "one@0", "none") else [])
            for out_r in outs:
                want = np.zeros((n, out_r), np.uint64)
                for r in on:
                    if r < out_r:
                        want[:, r] = pack_ref.unpack64(blob[int(off[r]):int(off[r] + ln[r])], n)
                out = np.full((n, out_r), FILL64, np.uint64)
                rc = L.rv_hook_unpack64(h, _p(blob), len(blob), _p(off), _p(ln), _p(omit), n, R, out_r, _p(out))
                what = f"k_unpack64, R = {R}, map {name}, n_items = {n}, out_r = {out_r}"
                assert rc == 0, f"{what}: error {rc}"
                if not np.array_equal(out, want):
                    pytest.fail(f"{what}: first wrong word: {pack_ref.first_diff_rows(out, want, per_quad=1)}")
    out = np.full((3, R), FILL64, np.uint64)
    z = np.zeros(R, np.uint64)
    assert L.rv_hook_unpack64(h, _p(np.zeros(8, np.uint8)), 8, _p(z), _p(z), _p(maps(R)["none"]), 0, R, R, _p(out)) == 0 and (out == FILL64).all()


# ---- the direct path: k_extract_rows<0> into a second buffer, then k_copy_gaps ----
POISON = 0x5A  # the image's broadcast vectors before the extraction


@functools.lru_cache(maxsize=None)
def _direct_case(n, rec_pad):
    """an image of 40 records and a tail: record j = head | vector (at 137) | 8 bytes | corrections | rec_pad bytes; noise everywhere
    but in the vectors, which come from the reference"""
    R = 256
    omit = maps(R)["scattered"]
    rng = np.random.default_rng(n)
    pool = _row_stream(R, 0, 257, 140)
    ids = rng.integers(0, len(pool), n).astype(np.uint32)
    vecs = pack_ref.pack_rows(pool, omit, 0, ids)
    nb = pack_ref.n_bytes(n)
    first, rvec_at, corr_len = 40, 137, nb // 3 + 5
    corr_at = rvec_at + nb + 8
    rec = corr_at + corr_len + rec_pad
    total = first + 40 * rec + 216 * 48 + 3
    img = rng.integers(0, 256, total, dtype=np.uint8)
    at = np.zeros(R, np.uint64)
    for j, r in enumerate(pack_ref.opened(omit)):
        at[r] = first + j * rec + rvec_at
        img[int(at[r]):int(at[r]) + nb] = vecs[r]
    img.setflags(write=False)
    return omit, pool, ids, at, img, (first, rec, corr_at, corr_len, rvec_at, nb)


@pytest.mark.parametrize("n,rec_pad,want_tile", [
    (8 * 32767 + 3, 8, 16),     # vectors of 32768 bytes (0 mod 16), records 8 mod 16 apart: starts of two alignments
    (8 * 32770 + 5, 5, 16),     # 32771 bytes (3 mod 16), record size odd: starts of every alignment mod 16
    (8 * 65600, 1, 32),
    (8 * 300 + 1, 4, 8),        # tile 8: k_copy_gaps takes no OpenDirect, the extraction still writes its words
], ids=["len0mod16", "len3mod16", "tile32", "tile8"])
def test_direct_path(hooks, n, rec_pad, want_tile):
    omit, pool, ids, at, img, (first, rec, corr_at, corr_len, rvec_at, nb) = _direct_case(n, rec_pad)
    starts = {int(a) % 16 for a in at[omit < 8]}
    assert len(starts) == (16 if rec % 2 else 2)
    n_tiles = (nb + want_tile - 1) // want_tile
    on = pack_ref.opened(omit)
    spans = [(r, int(at[r]), nb) for r in on]
    for rep_limit in (256, 120):
        m = sum(1 for r in on if r < rep_limit)
        assert 0 < m < 40 or rep_limit == 256
        for n_direct in (0, 1, n_tiles, n_tiles + 7):
            for with_od in ((0, 1) if n_direct else (0,)):
                src = img.copy()
                for r in on:
                    src[int(at[r]):int(at[r]) + nb] = POISON
                dst = np.full(len(img), FILL, np.uint8)
                gaps = _u64([first, rec, corr_at, corr_len, 40, rep_limit, rvec_at, with_od])
                rc, tile = call_extract_bits(hooks, pool, ids, n, 256, 0, omit, at, src, dst, n_direct, gaps)
                what = (f"k_extract_rows<0> + k_copy_gaps, n_items = {n}, tile {tile}, n_direct = {n_direct} of {n_tiles} tiles, "
                        f"{'with' if with_od else 'without'} OpenDirect, rep_limit = {rep_limit}, record size {rec}")
                assert rc == 0, f"{what}: error {rc}"
                assert tile == want_tile, what
                if not np.array_equal(src, img):
                    pytest.fail(f"{what}: the image: first wrong byte: {pack_ref.first_diff_bytes(src, img, spans)}")
                want = img.copy()
                for j in range(m):
                    want[first + j * rec + corr_at:first + j * rec + corr_at + corr_len] = FILL
                if not np.array_equal(dst, want):
                    x = int(np.nonzero(dst != want)[0][0])
                    j, o = divmod(x - first, rec)
                    pytest.fail(f"{what}: the second buffer: first wrong byte at offset {x} (record {j}, byte {o}; vector at [{rvec_at}, "
                                f"{rvec_at + nb}), corrections at [{corr_at}, {corr_at + corr_len})): got 0x{dst[x]:02x}, want 0x{want[x]:02x}; "
                                f"{pack_ref.first_diff_bytes(dst, want, spans)}")


# ---- what the hooks refuse: the right code before any launch, the buffers untouched ----
def _reject_args(R=32):
    omit = _with_players([1, 6, 30], R, 9).copy()
    return {"R": R, "omit": omit, "at": _u64(np.arange(R) * 16), "n": 40}


REJECTS = ["R12", "R264", "omit9", "opened41", "vector-outside", "row-outside", "direct-kind1", "gaps-outside",
           "bits-R12", "bits-omit9", "bits-opened41", "corr-pitch64", "corr-pitch-short",
           "unpack-R12", "unpack-omit9", "unpack-opened41", "unpack-nq16-late-rep", "unpack-nq8", "unpack-src-outside",
           "z64-R12", "z64-omit9", "z64-opened41", "z64-offset-outside", "unpack64-r64-late-rep", "unpack64-r32", "unpack64-omit9"]


@pytest.mark.parametrize("case", REJECTS)
def test_pack_hook_rejects(hooks, case):
    L, h = hooks
    a = _reject_args(256 if ("41" in case or "late" in case or case in ("unpack-nq8", "unpack64-r32")) else 32)
    R, omit, at, n = a["R"], a["omit"], a["at"], a["n"]
    if case.endswith("R12"):
        R = 12
    if case.endswith("R264"):
        R = 264
        omit, at = np.full(264, 8, np.uint8), _u64(np.zeros(264))
    if case.endswith("omit9"):
        omit[R - 1] = 9
    if case.endswith("opened41"):
        omit[100:141] = 3
        omit[[1, 6, 30]] = 8
    if case.endswith("late-rep"):
        omit[64] = 2
    out = np.full(1 << 14, FILL, np.uint8)
    out2 = np.full(1 << 14, FILL, np.uint8)
    tile = C.c_uint32(0)
    stream = np.zeros((64, 64), np.uint32)
    bits = np.zeros((64, 32), np.uint8)
    z = _u64(np.zeros(264))
    if case in ("R12", "R264", "omit9", "opened41", "vector-outside", "row-outside", "direct-kind1", "gaps-outside"):
        rows, kind, n_direct, gaps, size = None, 0, 0, None, len(out)
        if case == "vector-outside":
            at[30] = len(out) - 5
        if case == "row-outside":
            rows = np.arange(n, dtype=np.uint32)
            rows[7] = 64
        if case == "direct-kind1":
            kind, n_direct = 1, 1
        if case == "gaps-outside":
            gaps = _u64([40, 1000, 200, 100, 40, 256, 137, 0])  # 40 records of 1000 bytes in 16 KiB
        rc = L.rv_hook_extract_bits(h, _p(stream), 64, _p(rows), n, R, kind, _p(omit), _p(at), _p(out), size, _p(out2), n_direct, _p(gaps), C.byref(tile))
    elif case.startswith("bits-"):
        rc = L.rv_hook_extract_from_bits(h, _p(bits), n, R, _p(omit), _p(at), 0, _p(out), len(out), C.byref(tile))
    elif case.startswith("corr-"):
        pitch, n_b = (64, 8) if case == "corr-pitch64" else (128, 129)
        rc = L.rv_hook_pack_corr_all(h, _p(bits), 64, 0, n_b, pitch, _p(out))
    elif case.startswith("unpack-"):
        out_nq = {"unpack-nq16-late-rep": 16, "unpack-nq8": 8}.get(case, R // 4)
        ln = _u64(np.full(264, 6))
        if case == "unpack-src-outside":
            z[6] = 60
        rc = L.rv_hook_unpack_bits(h, _p(bits), 64, _p(z), _p(ln), _p(omit), n, R, 0, out_nq, 0, _p(out))
    elif case.startswith("z64-"):
        offs = None
        if case == "z64-offset-outside":
            offs = _u64(np.arange(8))
            offs[3] = 32 - 6  # + omit[6] = 7: past the stride of 32 words
            omit[6] = 7
        rc = L.rv_hook_extract64(h, _p(stream), 32, _p(offs), 8, 1, R, _p(omit), _p(at), 1, 0, _p(out), len(out))
    else:
        out_r = {"unpack64-r64-late-rep": 64, "unpack64-r32": 32}.get(case, R)
        rc = L.rv_hook_unpack64(h, _p(bits), 64, _p(z), _p(_u64(np.full(264, 8))), _p(omit), 4, R, out_r, _p(out))
    assert rc == E_ARG, f"{case}: returned {rc}"
    assert (out == FILL).all() and (out2 == FILL).all() and tile.value == 0
