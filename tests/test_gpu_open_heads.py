"""The kernels that decide WHAT a proof opens and WHERE every record lies -- k_fs_challenge, k_open_headers, k_open_small,
k_frame_counts and the set-up kernels k_overlay_rows, k_fill_digests, k_shard_init, k_store_words (open.hip) -- one production launch
at a time against tests/fs_ref.py and tests/pack_ref.py, byte for byte.

A whole proof feeds these kernels only what a real transcript hash yields, at the sizes one circuit fixes; here the challenge runs
on the named digest sets of tests/fs_cases.py (a shard that opens nothing, a crowded one, opened neighbours across the 64-lane
groups, re-drawn repetitions) at every shard form, section arithmetic past 2^32, every nullable output null and real, the
host-mapped mailbox, and a recorded batch; the heads at shuffled offsets and lengths whose second and third byte are not zero;
k_open_small in both forms up to its seam of 2 048 workgroups; one chain from digests to a parsed proof.

The rv_hook_* entry points (csrc/hooks_open.inc) call the production launch_* functions unchanged and return every output buffer
whole; outputs start as 0xA5 and a byte outside the expected ones must still be 0xA5.  tests/test_fs_ref_host.py ties the
reference to the CPU oracle and a golden proof.

Not tested: the second draw round of k_fs_challenge.  The second draw round needs fewer than 40 distinct values among 128 draws. No
input is known, and none is to be hunted for."""
import ctypes as C
import functools

import numpy as np
import pytest

import fs_cases
import fs_ref
import pack_ref
import proof_mutate
from test_gpu_pack import maps, tile_length

pytestmark = pytest.mark.gpu

FILL = 0xA5
FILL32 = 0xA5A5A5A5
FILL64 = 0xA5A5A5A5A5A5A5A5
FILL_INT = FILL32 - (1 << 32)  # the fill as a C int
E_ARG = 9
OL_BYTES, OL_REP, OL_DST = 488, 4, 168  # the kernel's list of opened repetitions: u32 n | u32 rep[40] | 4 bytes of padding | u64 dst[40]


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


def ol_bytes(ol):
    """the list as the kernel leaves it in a buffer of fill bytes: entries at and above n untouched"""
    b = np.full(OL_BYTES, FILL, np.uint8)
    b[0:4] = np.frombuffer(np.uint32(ol["n"]).tobytes(), np.uint8)
    n = len(ol["rep"])
    b[OL_REP:OL_REP + 4 * n] = np.asarray(ol["rep"], "<u4").view(np.uint8)
    b[OL_DST:OL_DST + 8 * n] = np.asarray(ol["dst"], "<u8").view(np.uint8)
    return b


OL_FIELDS = [("n", 0, 4)] + [(f"rep[{k}]", OL_REP + 4 * k, 4) for k in range(40)] + [("padding", 164, 4)] + [(f"dst[{k}]", OL_DST + 8 * k, 8) for k in range(40)]


# ------------------------------------------------------------------------------------
# k_fs_challenge
# ------------------------------------------------------------------------------------
SHARD_FORMS = [(0, 256), (0, 128), (128, 128), (64, 64), (192, 64), (0, 32), (96, 32), (224, 32), (120, 8)]  # 8: the smallest shard
# (name, lens = l2r l2c l2i l64r l64c l64i, base[0]); "huge": sz2 and sz64 exceed 2^32 (numbers only: no memory lies behind them)
LAYOUTS = [
    ("1-1|0-0", (1, 1, 1, 0, 0, 0), 0),
    ("odd@5", (3, 130, 2, 8, 16, 24), 5),
    ("odd@40", (7, 33, 5, 24, 8, 16), 40),
    ("huge", (2**33 + 3, 9, 2, 2**34 + 8, 16, 8), 0),
]
UNUSED_BASE = 2**35 + 12345  # base[1..3] of an unframed layout: the kernel must not use them
F_ALL, F_RES, F_COMM2, F_MBOX = 1, 2, 4, 8


@functools.lru_cache(maxsize=None)
def _expected_layout(name, rb, R, lens, base0, framed):
    omit = fs_cases.case(name)[2]
    return fs_ref.layout(omit[rb:rb + R], lens, base0, framed)


def fs_layout_words(lens, base0, framed):
    sz2, sz64 = fs_ref.record_sizes(lens)
    base = fs_ref.section_starts(40, 216, lens, base0, True)[0] if framed else [base0] + [UNUSED_BASE + k for k in range(3)]
    return _u64(list(base) + [sz2, sz64, lens[0], lens[1], lens[3], lens[4]])


def call_fs(hooks, digests, lens, base0, framed, rb, R, flags, seq=0, batch=0):
    L, h = hooks
    B = max(batch, 1)
    out = {
        "comm": np.full((B, 32), FILL, np.uint8), "omit": np.full((B, R), FILL, np.uint8), "omit_all": np.full((B, 256), FILL, np.uint8),
        "offs": np.full((B, 8, R), FILL64, np.uint64), "ol": np.full((B, OL_BYTES), FILL, np.uint8), "res": np.full((B, 2), FILL32, np.uint32),
        "comm2": np.full((B, 32), FILL, np.uint8), "mbox": np.full(128, FILL32, np.uint32),
    }
    digests = np.ascontiguousarray(digests, np.uint8)
    assert digests.size == B * 8192
    rc = L.rv_hook_fs_challenge(h, _p(digests), _p(fs_layout_words(lens, base0, framed)), int(framed), rb, R, flags, seq, batch, _p(out["comm"]), _p(out["omit"]),
                                _p(out["omit_all"]), _p(out["offs"]), _p(out["ol"]), _p(out["res"]), _p(out["comm2"]), _p(out["mbox"]))
    return rc, out


def check_fs(out, b, name, lens, base0, framed, rb, R, flags, seq, what):
    _, comm, omit, _, _ = fs_cases.case(name)
    table, ol, (n_on, n_pre), _ = _expected_layout(name, rb, R, tuple(lens), base0, framed)
    what = f"k_fs_challenge, digests {name}, shard ({rb}, {R}) with {n_on} opened, {what}, flags {flags}"
    assert out["comm"][b].tobytes() == comm.tobytes(), f"{what}: comm"
    if not np.array_equal(out["omit"][b], omit[rb:rb + R]):
        r = int(np.nonzero(out["omit"][b] != omit[rb:rb + R])[0][0])
        pytest.fail(f"{what}: omit[{r}] (repetition {rb + r}) is {out['omit'][b][r]}, want {omit[rb + r]}")
    want_all = omit if flags & F_ALL else np.full(256, FILL, np.uint8)
    assert np.array_equal(out["omit_all"][b], want_all), f"{what}: omit_all, first at {np.nonzero(out['omit_all'][b] != want_all)[0][:1]}"
    if not np.array_equal(out["offs"][b], table):
        j, r = (int(x) for x in np.argwhere(out["offs"][b] != table)[0])
        rows = ("gf2 record", "z64 record", "gf2 rec", "gf2 corr", "gf2 in", "z64 rec", "z64 corr", "z64 in")
        pytest.fail(f"{what}: table row {j} ({rows[j]}), local repetition {r} (omit {omit[rb + r]}): got {int(out['offs'][b][j, r])}, want {int(table[j, r])}")
    want_ol = ol_bytes(ol)
    if not np.array_equal(out["ol"][b], want_ol):
        pytest.fail(f"{what}: the list of opened repetitions: {fs_ref.describe(out['ol'][b], want_ol, OL_FIELDS)}")
    assert out["res"][b].tolist() == ([n_on, n_pre] if flags & F_RES else [FILL32, FILL32]), f"{what}: res"
    assert out["comm2"][b].tobytes() == (comm.tobytes() if flags & F_COMM2 else bytes([FILL]) * 32), f"{what}: comm2"
    want_mbox = np.full(128, FILL32, np.uint32)
    if flags & F_MBOX:
        want_mbox[0] = seq
        want_mbox[16:90] = fs_ref.mailbox(comm, omit, n_on, n_pre)
    if not np.array_equal(out["mbox"], want_mbox):
        w = int(np.nonzero(out["mbox"] != want_mbox)[0][0])
        pytest.fail(f"{what}: mailbox word {w} (0: stamp, 16..23 comm, 24..87 the map, 88, 89 the counts): got 0x{out['mbox'][w]:08x}, want 0x{want_mbox[w]:08x}")


def forms_of(name):
    own = fs_cases.own_shard(name, fs_cases.case(name)[2])
    return SHARD_FORMS + ([own] if own and own not in SHARD_FORMS else [])


@pytest.mark.parametrize("name", fs_cases.NAMES)
def test_fs_challenge(hooks, name):
    """every shard form x every layout, unframed and (the whole shard) framed; the nullable outputs null and real in turn"""
    digests = fs_cases.digests(name)
    turn = 0
    for rb, R in forms_of(name):
        cases = [(ln, lens, base0, False) for ln, lens, base0 in LAYOUTS]
        if (rb, R) == (0, 256):
            cases += [(ln + ", framed", lens, 0, True) for ln, lens, _ in LAYOUTS]
        for ln, lens, base0, framed in cases:
            flags = [F_ALL | F_RES | F_COMM2, 0, F_ALL, F_RES, F_COMM2, F_ALL | F_RES][turn % 6] | (F_COMM2 if framed else 0)
            turn += 1
            rc, out = call_fs(hooks, digests, lens, base0, framed, rb, R, flags)
            assert rc == 0, f"digests {name}, shard ({rb}, {R}), layout {ln}: error {rc}"
            check_fs(out, 0, name, lens, base0, framed, rb, R, flags, 0, f"layout {ln}")


@pytest.mark.parametrize("seq", [1, 0x7FFFFFF3])
def test_fs_challenge_mailbox(hooks, seq):
    """the early path's host-mapped mailbox: comm, the whole map, the shard's counts, then the stamp"""
    for name, (rb, R), framed in (("plain", (0, 256), True), ("crowded32", fs_cases.own_shard("crowded32", fs_cases.case("crowded32")[2]), False),
                                  ("empty32@3", (96, 32), False), ("seam127", (0, 128), False)):
        _, lens, base0 = LAYOUTS[1]
        for flags in (F_MBOX, F_MBOX | F_ALL | F_RES | F_COMM2):
            flags |= F_COMM2 if framed else 0
            rc, out = call_fs(hooks, fs_cases.digests(name), lens, 0 if framed else base0, framed, rb, R, flags, seq=seq)
            assert rc == 0
            check_fs(out, 0, name, lens, 0 if framed else base0, framed, rb, R, flags, seq, f"mailbox with stamp {seq}")


@pytest.mark.parametrize("form", [(0, 256), (64, 64), (0, 32)])
def test_fs_challenge_recorded_batch(hooks, form):
    """three different digest sets recorded and replayed as one batch (k_many): every proof of the batch gets its own answer"""
    names = ["crowded64", "empty32@0", "seam63"]
    digests = np.stack([fs_cases.digests(n) for n in names])
    rb, R = form
    for (ln, lens, base0), flags in zip(LAYOUTS, (F_ALL | F_RES | F_COMM2, 0, F_RES, F_ALL)):
        rc, out = call_fs(hooks, digests, lens, base0, False, rb, R, flags, batch=3)
        assert rc == 0, rc
        for b, name in enumerate(names):
            check_fs(out, b, name, lens, base0, False, rb, R, flags, 0, f"proof {b} of a recorded batch of 3, layout {ln}")


def call_fs_raw(hooks, digests, lens, framed, rb, R, flags, batch):
    """call_fs with output buffers sized for a whole shard whatever R says (the refused calls)"""
    L, h = hooks
    B = max(batch, 1)
    out = {"comm": np.full((B, 32), FILL, np.uint8), "omit": np.full((B, 256), FILL, np.uint8), "omit_all": np.full((B, 256), FILL, np.uint8),
           "offs": np.full((B, 8, 256), FILL64, np.uint64), "ol": np.full((B, OL_BYTES), FILL, np.uint8), "res": np.full((B, 2), FILL32, np.uint32),
           "comm2": np.full((B, 32), FILL, np.uint8), "mbox": np.full(128, FILL32, np.uint32)}
    rc = L.rv_hook_fs_challenge(h, _p(digests), _p(fs_layout_words(lens, 0, framed)), int(framed), rb, R, flags, 0, batch, _p(out["comm"]), _p(out["omit"]),
                                _p(out["omit_all"]), _p(out["offs"]), _p(out["ol"]), _p(out["res"]), _p(out["comm2"]), _p(out["mbox"]))
    return rc, out


@pytest.mark.parametrize("case", ["R12", "R0", "begin4", "past-end", "framed-part", "mailbox-batch", "batch1", "flags16", "size-2^37"])
def test_fs_challenge_rejects(hooks, case):
    rb, R, framed, flags, batch, lens = 0, 32, False, 7, 0, LAYOUTS[1][1]
    if case == "R12":
        R = 12
    if case == "R0":
        R = 0
    if case == "begin4":
        rb = 4
    if case == "past-end":
        rb, R = 192, 128
    if case == "framed-part":
        framed, R = True, 128
    if case == "mailbox-batch":
        flags, batch = F_MBOX, 2
    if case == "batch1":
        batch = 1
    if case == "flags16":
        flags = 16
    if case == "size-2^37":
        lens = (2**37, 1, 1, 0, 0, 0)
    B = max(batch, 1)
    digests = np.stack([fs_cases.digests("plain")] * B)
    rc, out = call_fs_raw(hooks, digests, lens, framed, rb, R, flags, batch)
    assert rc == E_ARG, f"{case}: returned {rc}"
    for k, v in out.items():
        assert (v == (FILL if v.dtype == np.uint8 else FILL32 if v.dtype == np.uint32 else FILL64)).all(), f"{case}: {k} was written"


# ------------------------------------------------------------------------------------
# k_open_headers
# ------------------------------------------------------------------------------------
HEAD_LENS = [(1, 1, 1, 0, 0, 0), (3, 130, 2, 8, 16, 24), (70001, 300, 1, 72000, 0, 8)]  # the last: length bytes 1 and 2 non-zero, three length fields touch


@functools.lru_cache(maxsize=None)
def shard_inputs(R, seed=0):
    """seeds [R][16], keys [R][128] (no zero byte: a key left in place shows), on2 / on64 [R][8] u32"""
    rng = np.random.default_rng([77, R, seed])
    arrs = (rng.integers(0, 256, (R, 16), dtype=np.uint8), rng.integers(1, 256, (R, 128), dtype=np.uint8),
            rng.integers(0, 2**32, (R, 8), dtype=np.uint64).astype(np.uint32), rng.integers(0, 2**32, (R, 8), dtype=np.uint64).astype(np.uint32))
    for a in arrs:
        a.setflags(write=False)
    return arrs


def shuffled_table(omit, lens, seed, base=5):
    """the shard's 2 R records side by side in a shuffled order from an odd base (as test_gpu_pack.layout lays vectors out)"""
    R = len(omit)
    sz = fs_ref.record_sizes(lens)
    order = np.random.default_rng(seed).permutation(2 * R)
    off, at = np.zeros((2, R), np.uint64), base
    for x in order:
        dom, r = divmod(int(x), R)
        off[dom, r] = at
        at += sz[dom] if omit[r] < 8 else 48
    return fs_ref.record_table(omit, off[0], off[1], lens), at


def check_image(got, pieces, omit, table, lens, what):
    want = fs_ref.image(FILL, len(got), pieces)
    if not np.array_equal(got, want):
        pytest.fail(f"{what}: {fs_ref.describe(got, want, fs_ref.fields(omit, table, lens))}")


@pytest.mark.parametrize("lens", HEAD_LENS, ids=["1-1-1|0-0-0", "3-130-2|8-16-24", "70001-300-1|72000-0-8"])
@pytest.mark.parametrize("R", [256, 32])
def test_open_headers(hooks, R, lens):
    L, h = hooks
    seeds, keys, on2, on64 = shard_inputs(R)
    if R == 256:
        assert set(maps(R)["scattered"][maps(R)["scattered"] < 8].tolist()) == set(range(8))  # every player is omitted somewhere
    for i, (name, omit) in enumerate(maps(R).items()):
        for order in ("production order from 0", "shuffled from an odd base"):
            if order.startswith("production"):
                table, _, _, end = fs_ref.layout(omit, lens, 0, False)
            else:
                table, end = shuffled_table(omit, lens, 10 * R + i)
            out = np.full(end + 9, FILL, np.uint8)
            rc = L.rv_hook_open_headers(h, R, _p(omit), _p(seeds), _p(keys), _p(on2), _p(on64), _p(_u64(table[0])), _p(_u64(table[1])), _p(_u64(lens)), _p(out), len(out))
            what = f"k_open_headers, R = {R}, map {name}, lengths {lens}, records in {order}"
            assert rc == 0, f"{what}: error {rc}"
            check_image(out, fs_ref.heads(omit, seeds, keys, on2, on64, table, lens), omit, table, lens, what)


def test_open_headers_rejects(hooks):
    L, h = hooks
    R, lens = 32, HEAD_LENS[1]
    omit = maps(R)["scattered"]
    seeds, keys, on2, on64 = shard_inputs(R)
    table, _, _, end = fs_ref.layout(omit, lens, 0, False)
    for case, (size, om) in {"record-outside": (end - 1, omit), "omit9": (end, np.where(np.arange(R) == 3, 9, omit).astype(np.uint8))}.items():
        out = np.full(end, FILL, np.uint8)
        rc = L.rv_hook_open_headers(h, R, _p(om), _p(seeds), _p(keys), _p(on2), _p(on64), _p(_u64(table[0])), _p(_u64(table[1])), _p(_u64(lens)), _p(out), size)
        assert rc == E_ARG and (out == FILL).all(), case


# ------------------------------------------------------------------------------------
# k_open_small
# ------------------------------------------------------------------------------------
def call_open_small(hooks, R, omit, table, lens, stream, rec_rows, n_rec, pre, n_pre, in_rows, n_in, ol, rep_min, err_src, flags, out, err_word=FILL_INT):
    L, h = hooks
    seeds, keys, on2, on64 = shard_inputs(R)
    taken, word, tiles = C.c_int(-1), C.c_int(err_word), np.zeros(3, np.uint32)
    stream = np.ascontiguousarray(stream, np.uint32)
    rc = L.rv_hook_open_small(h, R, _p(omit), _p(seeds), _p(keys), _p(on2), _p(on64), _p(_u64(table)), _p(_u64(lens)), _p(stream), stream.shape[0], _p(rec_rows), n_rec,
                              _p(pre), n_pre, _p(in_rows), n_in, _p(ol), rep_min, err_src, flags, _p(out), len(out), C.byref(taken), _p(tiles), C.byref(word))
    return rc, taken.value, tiles.tolist(), word.value


def small_pieces(omit, table, lens, stream, rec_rows, pre, n_pre, in_rows, ol_reps, rep_min, heads_inputs_only):
    """what k_open_small leaves: the heads, the input vectors, and -- in the full form -- the broadcast vectors and the corrections
    vectors of the listed repetitions from rep_min on"""
    seeds, keys, on2, on64 = shard_inputs(len(omit))
    pieces = dict(fs_ref.heads(omit, seeds, keys, on2, on64, table, lens))
    vecs = [(4, pack_ref.pack_rows(stream, omit, 1, in_rows))]
    if not heads_inputs_only:
        vecs += [(2, pack_ref.pack_rows(stream, omit, 0, rec_rows)), (3, pack_ref.pack_bitstream(pre[:n_pre], [r for r in ol_reps if r >= rep_min]))]
    for row, vs in vecs:
        for r, v in vs.items():
            assert len(v) == lens[row - 2]
            pieces[int(table[row, r])] = v.tobytes()
    return pieces


@functools.lru_cache(maxsize=None)
def small_streams(R):
    rng = np.random.default_rng([88, R])
    stream = rng.integers(0, 2**32, (97, R // 4), dtype=np.uint64).astype(np.uint32)
    pre = rng.integers(0, 256, (80, R // 8), dtype=np.uint8)
    return stream, pre


def small_maps(R):
    out = {"scattered": maps(R)["scattered"], "one@end": maps(R)["one@end"]}
    if R == 32:
        for name in ("empty32@3", "crowded32"):
            omit = fs_cases.case(name)[2]
            rb, _ = fs_cases.own_shard(name, omit)
            out[name] = np.ascontiguousarray(omit[rb:rb + 32])
        assert (out["empty32@3"] == 8).all() and (out["crowded32"] < 8).sum() >= 13
    return out


COUNTS = [(0, 0, 0), (1, 7, 8), (7, 8, 9), (8, 9, 65), (9, 65, 1), (65, 1, 7), (65, 65, 65)]  # every count on every vector
ERR_FORMS = [(0, 0), (0, 2), (-7, 0), (0x1234, 2)]  # (err_src, flag bit 1: the host word is passed)


@pytest.mark.parametrize("only", [0, 1], ids=["full", "heads_inputs_only"])
@pytest.mark.parametrize("R", [256, 32])
def test_open_small(hooks, R, only):
    stream, pre = small_streams(R)
    rng = np.random.default_rng([R, only])
    turn = 0
    for name, omit in small_maps(R).items():
        for n_rec, n_pre, n_in in COUNTS:
            lens = (n_rec // 8 + 1, n_pre // 8 + 1, n_in // 8 + 1) + ((0, 0, 0) if turn % 2 else (8, 16, 24))
            table, ol, _, end = fs_ref.layout(omit, lens, 3 * (turn % 3), False)
            for rep_min in (0, R // 2, R):
                err_src, host = ERR_FORMS[turn % 4]
                listed = turn % 3 != 0
                turn += 1
                rec_rows = rng.integers(0, len(stream), n_rec).astype(np.uint32) if listed else None
                in_rows = rng.integers(0, len(stream), n_in).astype(np.uint32) if listed else None
                out = np.full(end + 7, FILL, np.uint8)
                rc, taken, tiles, word = call_open_small(hooks, R, omit, table, lens, stream, rec_rows, n_rec, pre, n_pre, in_rows, n_in, ol_bytes(ol), rep_min,
                                                         err_src, only | host, out)
                what = (f"k_open_small ({'heads and inputs only' if only else 'full'}), NQ = {R // 4}, map {name}, items {n_rec}, {n_pre}, {n_in}, corr_rep_min = {rep_min}, "
                        f"{'row lists' if listed else 'rows in order'}, err_src = {err_src}, host word {'passed' if host else 'null'}")
                assert rc == 0, f"{what}: error {rc}"
                assert taken == 1 and tiles == [8, 8, 8], f"{what}: taken {taken}, tiles {tiles}"
                assert word == (err_src if host else FILL_INT), f"{what}: the host's error word is {word}"
                ids = lambda rows, n: np.arange(n) if rows is None else rows  # noqa: E731
                pieces = small_pieces(omit, table, lens, stream, ids(rec_rows, n_rec), pre, n_pre, ids(in_rows, n_in), ol["rep"], rep_min, only)
                check_image(out, pieces, omit, table, lens, what)


@pytest.mark.parametrize("err", ERR_FORMS, ids=["zero-null", "zero-host", "nonzero-null", "nonzero-host"])
def test_open_small_error_word(hooks, err):
    """the error word rides along in both forms, whatever the device word holds, and only when the host's word is passed"""
    R = 32
    err_src, host = err
    stream, pre = small_streams(R)
    omit = small_maps(R)["crowded32"]
    lens = (2, 2, 2, 0, 0, 0)
    table, ol, _, end = fs_ref.layout(omit, lens, 0, False)
    for only in (0, 1):
        out = np.full(end, FILL, np.uint8)
        rc, taken, _, word = call_open_small(hooks, R, omit, table, lens, stream, None, 9, pre, 9, None, 9, ol_bytes(ol), 0, err_src, only | host, out)
        assert (rc, taken) == (0, 1) and word == (err_src if host else FILL_INT)
        check_image(out, small_pieces(omit, table, lens, stream, np.arange(9), pre, 9, np.arange(9), ol["rep"], 0, only), omit, table, lens, f"error word {err}, only = {only}")


def test_open_small_seam(hooks):
    """the three ranges total exactly 2 048 workgroups: taken and correct; one more workgroup: declined, nothing written"""
    R = 32
    omit = small_maps(R)["crowded32"]
    rng = np.random.default_rng(2048)
    stream = small_streams(R)[0]
    nb = (8 * 1000, 8 * 1000, 8 * 48)  # vector bytes: 1000 + 1000 + 48 workgroups at tile 8
    assert all(b < tile_length(16, 128, 0) // 8 for b in nb)  # (shorter than the shortest vector that takes tile 16: ex_tb_for stays at 8)
    n_rec, n_pre, n_in = 8 * (nb[0] - 1) + 3, 8 * (nb[1] - 1), 8 * (nb[2] - 1) + 7
    pre = rng.integers(0, 256, (n_pre, R // 8), dtype=np.uint8)
    rec_rows = rng.integers(0, len(stream), n_rec).astype(np.uint32)
    for extra, want_taken in ((0, 1), (64, 0)):
        n_in_x = n_in + extra
        in_rows = rng.integers(0, len(stream), n_in_x).astype(np.uint32)
        lens = (n_rec // 8 + 1, n_pre // 8 + 1, n_in_x // 8 + 1, 0, 0, 0)
        table, ol, _, end = fs_ref.layout(omit, lens, 0, False)
        out = np.full(end + 5, FILL, np.uint8)
        rc, taken, tiles, word = call_open_small(hooks, R, omit, table, lens, stream, rec_rows, n_rec, pre, n_pre, in_rows, n_in_x, ol_bytes(ol), 0, 5, 2, out)
        groups = sum((ln + t - 1) // t for ln, t in zip(lens[:3], tiles))
        assert rc == 0 and tiles == [8, 8, 8] and groups == 2048 + (1 if extra else 0), (rc, tiles, groups)
        assert taken == want_taken, f"{groups} workgroups: taken = {taken}"
        if taken:
            assert word == 5
            check_image(out, small_pieces(omit, table, lens, stream, rec_rows, pre, n_pre, in_rows, ol["rep"], 0, 0), omit, table, lens, "k_open_small at 2048 workgroups")
        else:
            assert (out == FILL).all() and word == FILL_INT, "a declined launch wrote something"


@pytest.mark.parametrize("case", ["vector-outside", "list-outside", "row-outside", "list-n41", "list-rep-outside", "opened41", "rep_min-above-R", "head-outside"])
def test_open_small_rejects(hooks, case):
    R = 32
    stream, pre = small_streams(R)
    omit = small_maps(R)["scattered"].copy()
    lens = (2, 2, 2, 0, 0, 0)
    table, ol, _, end = fs_ref.layout(omit, lens, 0, False)
    table, olb, rows, rep_min, size = table.copy(), ol_bytes(ol), None, 0, end
    on = pack_ref.opened(omit)
    if case == "vector-outside":
        table[4, on[-1]] = end - 1
    if case == "list-outside":
        olb[OL_DST:OL_DST + 8] = np.frombuffer(np.uint64(end - 1).tobytes(), np.uint8)
    if case == "row-outside":
        rows = np.arange(9, dtype=np.uint32)
        rows[4] = len(stream)
    if case == "list-n41":
        olb[0] = 41
    if case == "list-rep-outside":
        olb[OL_REP:OL_REP + 4] = np.frombuffer(np.uint32(R).tobytes(), np.uint8)
    if case == "opened41":
        R, omit = 256, np.where(np.arange(256) < 41, 3, 8).astype(np.uint8)
        table = np.zeros((8, 256), np.uint64)
    if case == "rep_min-above-R":
        rep_min = R + 1
    if case == "head-outside":
        size = end - 1
    out = np.full(end, FILL, np.uint8)
    rc, taken, tiles, word = call_open_small(hooks, R, omit, table, lens, stream if R == 32 else small_streams(256)[0], rows, 9, pre if R == 32 else small_streams(256)[1], 9,
                                             None, 9, olb, rep_min, 1, 2, out[:size])
    assert rc == E_ARG and taken == -1 and tiles == [0, 0, 0] and word == FILL_INT and (out == FILL).all(), case


# ------------------------------------------------------------------------------------
# k_frame_counts
# ------------------------------------------------------------------------------------
def section_lengths(lens):
    sz2, sz64 = fs_ref.record_sizes(lens)
    return [40 * sz2, 216 * 48, 40 * sz64, 216 * 48]


def call_frame_counts(hooks, out, stride, batch, lens4):
    L, h = hooks
    taken = C.c_int(-1)
    rc = L.rv_hook_frame_counts(h, _p(out), len(out), stride, batch, _p(_u64(lens4)), C.byref(taken))
    return rc, taken.value


@pytest.mark.parametrize("lens", [(1, 1, 1, 0, 0, 0), (3, 130, 2, 8, 16, 24)], ids=["1-1-1|0-0-0", "3-130-2|8-16-24"])
@pytest.mark.parametrize("batch", [1, 3, 64, 65])
def test_frame_counts(hooks, batch, lens):
    total = fs_ref.section_starts(40, 216, lens, 0, True)[1]
    stride = (total + 255) // 256 * 256
    for st in ([stride, 0] if batch == 1 else [stride]):  # (one proof: production passes a stride of 0)
        out = np.full(batch * stride, FILL, np.uint8)
        rc, taken = call_frame_counts(hooks, out, st, batch, section_lengths(lens))
        assert (rc, taken) == (0, 1), (rc, taken)
        want = np.full(batch * stride, FILL, np.uint8)
        frame = {at: b for at, b in fs_ref.frame(bytes(32), 40, 216, lens).items() if at != 0}  # (the counts; comm is the challenge kernel's)
        assert sorted(len(b) for b in frame.values()) == [8] * 4
        for b in range(batch):
            for at, v in frame.items():
                want[b * stride + at:b * stride + at + 8] = np.frombuffer(v, np.uint8)
        if not np.array_equal(out, want):
            x = int(np.nonzero(out != want)[0][0])
            pytest.fail(f"k_frame_counts, batch {batch}, stride {st}: first wrong byte at offset {x} = proof {x // stride}, byte {x % stride} (the counts stand at "
                        f"{sorted(frame)}): got 0x{out[x]:02x}, want 0x{want[x]:02x}")


@pytest.mark.parametrize("case", ["length-4-mod-8", "stride-4-mod-8", "batch-0"])
def test_frame_counts_declines(hooks, case):
    """the launcher's own refusals: not taken, nothing written"""
    lens4 = section_lengths((3, 130, 2, 8, 16, 24))
    total = 32 + 4 * 8 + sum(lens4)
    stride, batch = (total + 255) // 256 * 256, 3
    if case == "length-4-mod-8":
        lens4[0] += 4
    if case == "stride-4-mod-8":
        stride += 4
    if case == "batch-0":
        batch = 0
    out = np.full(3 * stride + 8, FILL, np.uint8)
    rc, taken = call_frame_counts(hooks, out, stride, batch, lens4)
    assert (rc, taken) == (0, 0) and (out == FILL).all(), (case, rc, taken)


def test_frame_counts_rejects(hooks):
    lens4 = section_lengths((1, 1, 1, 0, 0, 0))
    total = 32 + 4 * 8 + sum(lens4)
    out = np.full(2 * total, FILL, np.uint8)
    for stride, batch, size in ((total, 3, 2 * total), (0, 1, total - 216 * 48 - 1)):  # the third proof / the last count outside the buffer
        taken = C.c_int(-1)
        rc = hooks[0].rv_hook_frame_counts(hooks[1], _p(out), size, stride, batch, _p(_u64(lens4)), C.byref(taken))
        assert rc == E_ARG and taken.value == -1 and (out == FILL).all()


# ------------------------------------------------------------------------------------
# the set-up kernels
# ------------------------------------------------------------------------------------
@pytest.mark.parametrize("row_words", [4, 8, 32, 33])
@pytest.mark.parametrize("R", [256, 32])
def test_overlay_rows(hooks, R, row_words):
    L, h = hooks
    rng = np.random.default_rng([R, row_words])
    src = rng.integers(0, 2**32, (R, row_words), dtype=np.uint64).astype(np.uint32)
    for name in ("none", "first", "scattered"):
        omit = maps(R)[name]
        for want_online in (0, 1):
            dst0 = rng.integers(0, 2**32, (R, row_words), dtype=np.uint64).astype(np.uint32)
            dst = dst0.copy()
            rc = L.rv_hook_overlay_rows(h, _p(dst), _p(src), _p(omit), R, row_words, want_online)
            assert rc == 0, rc
            want = np.where(((omit < 8) == bool(want_online))[:, None], src, dst0)
            if not np.array_equal(dst, want):
                r, w = (int(x) for x in np.argwhere(dst != want)[0])
                pytest.fail(f"k_overlay_rows, R = {R}, row_words = {row_words}, map {name}, want_online = {want_online}: row {r} (omit {omit[r]}), word {w}: "
                            f"got 0x{dst[r, w]:08x}, want 0x{want[r, w]:08x}")


FILL_ROWS = [1, 31, 32, 33, 256]
DIGEST = np.array([0x01020304, 0, 0xFFFFFFFF, 0x80000000, 5, 6, 0x7FFFFFFF, 0xA5A5A5A5], np.uint32)


def _want_fill(n_rows, words):
    want = np.full(words, FILL32, np.uint32)
    want[:8 * n_rows] = np.tile(DIGEST, n_rows)
    return want


@pytest.mark.parametrize("n_rows", FILL_ROWS)
def test_fill_digests(hooks, n_rows):
    L, h = hooks
    dst = np.full(8 * n_rows + 13, FILL32, np.uint32)
    assert L.rv_hook_fill_digests(h, _p(dst), len(dst), n_rows, _p(DIGEST)) == 0
    want = _want_fill(n_rows, len(dst))
    assert np.array_equal(dst, want), f"k_fill_digests, n_rows = {n_rows}: first wrong word {np.nonzero(dst != want)[0][:1]}"
    short = np.full(8 * n_rows - 1, FILL32, np.uint32)
    assert L.rv_hook_fill_digests(h, _p(short), len(short), n_rows, _p(DIGEST)) == E_ARG and (short == FILL32).all()


def call_shard_init(hooks, n_mask, n_corr, n_fill_rows, with_zero_byte):
    L, h = hooks
    err = np.full(2, FILL_INT, np.int32)
    mask, corr = np.full(80, FILL32, np.uint32), np.full(80, FILL, np.uint8)
    fill = None if n_fill_rows is None else np.full(8 * n_fill_rows + 13, FILL32, np.uint32)
    zero = np.full(8, FILL, np.uint8) if with_zero_byte else None
    rc = L.rv_hook_shard_init(h, _p(err), _p(mask), len(mask), n_mask, _p(corr), len(corr), n_corr, _p(fill), 0 if fill is None else len(fill), n_fill_rows or 0,
                              _p(DIGEST) if fill is not None else None, _p(zero))
    return rc, err, mask, corr, fill, zero


@pytest.mark.parametrize("n_fill_rows", [None] + FILL_ROWS)
def test_shard_init(hooks, n_fill_rows):
    for n_mask, n_corr in ((1, 1), (64, 64), (1, 64), (64, 1)):
        for with_zero_byte in (False, True):
            rc, err, mask, corr, fill, zero = call_shard_init(hooks, n_mask, n_corr, n_fill_rows, with_zero_byte)
            what = f"k_shard_init, {n_mask} mask words, {n_corr} corr bytes, {n_fill_rows} digest rows, zero_byte {'real' if with_zero_byte else 'null'}"
            assert rc == 0, f"{what}: error {rc}"
            assert err.tolist() == [0, FILL_INT], f"{what}: the error word"
            assert (mask[:n_mask] == 0).all() and (mask[n_mask:] == FILL32).all(), f"{what}: the zero row's mask words"
            assert (corr[:n_corr] == 0).all() and (corr[n_corr:] == FILL).all(), f"{what}: the zero row's corr bytes"
            if fill is not None:
                want = _want_fill(n_fill_rows, len(fill))
                assert np.array_equal(fill, want), f"{what}: digest word {np.nonzero(fill != want)[0][:1]}"
            if with_zero_byte:
                assert zero.tolist() == [0] + [FILL] * 7, f"{what}: zero_byte"


@pytest.mark.parametrize("n_mask,n_corr", [(65, 1), (1, 65), (65, 65)])
def test_shard_init_rejects_more_than_64(hooks, n_mask, n_corr):
    """the kernel has 64 threads and no loop: the hook refuses what it would silently leave undone"""
    rc, err, mask, corr, fill, zero = call_shard_init(hooks, n_mask, n_corr, 2, True)
    assert rc == E_ARG
    assert (err == FILL_INT).all() and (mask == FILL32).all() and (corr == FILL).all() and (fill == FILL32).all() and (zero == FILL).all()


@pytest.mark.parametrize("with_err", [0, 1])
@pytest.mark.parametrize("n_words", [1, 255, 256, 257])
def test_store_words(hooks, n_words, with_err):
    L, h = hooks
    src = np.random.default_rng(n_words).integers(0, 2**32, n_words, dtype=np.uint64).astype(np.uint32)
    dst = np.full(n_words + 5, FILL32, np.uint32)
    word = C.c_int(FILL_INT)
    rc = L.rv_hook_store_words(h, _p(src), n_words, _p(dst), len(dst), 0x1234, with_err, C.byref(word))
    assert rc == 0, rc
    want = np.concatenate([src, np.full(5, FILL32, np.uint32)])
    assert np.array_equal(dst, want), f"k_store_words, n_words = {n_words}: first wrong word {np.nonzero(dst != want)[0][:1]}"
    assert word.value == (0x1234 if with_err else FILL_INT)
    assert L.rv_hook_store_words(h, _p(src), n_words, _p(dst), n_words - 1, 0, 0, C.byref(word)) == E_ARG


# ------------------------------------------------------------------------------------
# one chain: digests -> challenge -> heads and vectors -> counts = a proof
# ------------------------------------------------------------------------------------
def test_chain_is_a_proof(hooks):
    """k_fs_challenge's own table and list feed k_open_small, k_frame_counts closes the frame: the buffer parses as a proof and equals
    the one fs_ref and pack_ref assemble from the same inputs"""
    R, name = 256, "plain"
    n_rec, n_pre, n_in = 70, 33, 9
    lens = (n_rec // 8 + 1, n_pre // 8 + 1, n_in // 8 + 1, 0, 0, 0)
    stream, pre = small_streams(R)
    rc, fs = call_fs(hooks, fs_cases.digests(name), lens, 0, True, 0, R, F_ALL | F_RES | F_COMM2)
    assert rc == 0
    check_fs(fs, 0, name, lens, 0, True, 0, R, F_ALL | F_RES | F_COMM2, 0, "the chain")
    total = fs_ref.section_starts(40, 216, lens, 0, True)[1]
    out = np.full(total, FILL, np.uint8)
    out[:32] = fs["comm2"][0]  # (production points comm2 at the head of the proof buffer)
    rc, taken, _, _ = call_open_small(hooks, R, fs["omit"][0], fs["offs"][0], lens, stream, None, n_rec, pre, n_pre, None, n_in, fs["ol"][0], 0, 0, 0, out)
    assert (rc, taken) == (0, 1)
    rc, taken = call_frame_counts(hooks, out, 0, 1, section_lengths(lens))
    assert (rc, taken) == (0, 1)
    # the reference's proof from the same inputs
    _, comm, omit, _, _ = fs_cases.case(name)
    table, ol, (n_on, n_pre_reps), end = fs_ref.layout(omit, lens, 0, True)
    assert end == total
    pieces = small_pieces(omit, table, lens, stream, np.arange(n_rec), pre, n_pre, np.arange(n_in), ol["rep"], 0, False)
    pieces.update(fs_ref.frame(comm, n_on, n_pre_reps, lens))
    want = fs_ref.image(FILL, total, pieces)
    assert sum(len(b) for b in pieces.values()) == total  # (a pure GF(2) proof: the z64 vectors are empty, every byte is some piece's)
    if not np.array_equal(out, want):
        pytest.fail(f"the chain's proof: {fs_ref.describe(out, want, [('comm', 0, 32)] + fs_ref.fields(omit, table, lens))}")
    got_comm, domains = proof_mutate.parse(out.tobytes())
    assert got_comm == comm.tobytes() and [len(d[0]) for d in domains] == [40, 40] and [len(d[1]) for d in domains] == [216 * 48] * 2
    assert [rec[0] for rec in domains[0][0]] == [int(omit[r]) for r in ol["rep"]]
    assert proof_mutate.serialise(got_comm, domains) == out.tobytes()
