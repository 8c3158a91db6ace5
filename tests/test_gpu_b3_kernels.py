"""The transcript-hash kernels -- the byte-row, bit-row and contiguous-stream chunk kernels, the paired chunk kernels, the tree
reductions and tops, the streaming prover's incremental tree and the digest join (b3_tree.hip; z64.hip: k_b3_chunks_contig) -- one
production launch at a time against tests/b3_ref.py, bit for bit: at event counts on every block and chunk edge, at every row width, at
chunk counters on both sides of 2^32, under quad lists, at every tree size that takes another path, directly and as a recorded batch.

The rv_hook_b3_* entry points call the production launch functions, with production's own choice of kernel (choice = 0) or with a forced
one through the launch code production runs after choosing, so every kernel is reached at small shapes; tests/test_b3_plan_host.py pins
the choices.  Outputs start as 0xA5 and come back whole: a word the reference does not define -- a skipped quad word's chaining value,
anything behind the last chaining value or digest -- must still be 0xA5A5A5A5.  tests/test_b3_ref_host.py ties the reference to the
official BLAKE3, and test_end_to_end below ties the layout helpers to it.

Not tested: a natural (unforced) pick of the chunk-per-wavefront kernels through the hooks -- 2 048 chunks at NQ = 64 are 512 MiB of
rows; the plan test and the mid-size proof tests cover that seam.  A forced tree top can only be asked for the nodes the reductions
leave (at most 512), so "the 512-node top with more than 512 nodes" cannot be expressed; the hooks refuse the other misfits."""
import ctypes as C
import functools

import numpy as np
import pytest

import b3_ref

pytestmark = pytest.mark.gpu

FILL32 = 0xA5A5A5A5
PAD = 40  # words behind every output that must come back untouched
E_ARG = 9
RPL1, RPL4, UNI = 1, 2, 3
LANE, TAIL64, TAIL512 = 1, 2, 3
PAIR_Q, PAIR_LANE = 1, 2
# the empty stream, a partial and an exact first block, an exact chunk, a last chunk of one event, a last chunk ending in a partial block
COUNTS = [0, 1, 63, 64, 65, 127, 128, 1023, 1024, 1025, 1087, 1088, 2047, 2048, 2049, 4072]
FEW = [0, 65, 1025, 4072]
QCOLS = [15, 16, 17, 47, 48, 49]  # k_b3_chunks_pair_q: a lane loads one of four columns of 16 rows
BASES = [0, 1, 2**32 - 1, 2**40 + 5]


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


@pytest.fixture(scope="module")
def hooks():
    import reverie_amd
    from reverie_amd import _lib

    ctx = reverie_amd.Context.default()  # raises loudly if the HIP library or the GPU is missing
    return _lib.lib(), ctx.handle


def same(got, want, what):
    """bit for bit; names the first differing value [.., node, repetition]"""
    assert got.shape == want.shape, (what, got.shape, want.shape)
    if not np.array_equal(got, want):
        bad = np.argwhere((got != want).any(axis=-1))
        at = tuple(bad[0])
        pytest.fail(f"{what}: {len(bad)} of {want[..., 0].size} values differ, first at {at}: got {[hex(x) for x in got[at]]} want {[hex(x) for x in want[at]]}")


def frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays if len(arrays) > 1 else arrays[0]


# ---- inputs and their reference values: computed once, shared, read-only ----
@functools.lru_cache(maxsize=None)
def byte_case(R, n, seed=0):
    """(byte strings [R, n], device rows [n][R / 4])"""
    data = np.random.default_rng([1, R, n, seed]).integers(0, 256, (R, n), dtype=np.uint8)
    return frozen(data, b3_ref.byte_rows(data))


@functools.lru_cache(maxsize=None)
def byte_cvs(R, n, seed=0, base=0, root_ok=True):
    return frozen(b3_ref.chunk_cvs(byte_case(R, n, seed)[0], base, root_ok))


@functools.lru_cache(maxsize=None)
def bit_case(R, n, seed=0):
    """(bytes hashed [R, n], device rows [n][R / 8]): random bits with the all-zero and the all-one row, and an all-zero and an
    all-one repetition, among them"""
    bits = np.random.default_rng([2, R, n, seed]).integers(0, 2, (R, n), dtype=np.uint8)
    bits[0], bits[R - 1] = 0, 1
    if n >= 2:
        bits[:, n // 3] = 0
        bits[:, n // 3 + 1] = 1
    rows, hashed = b3_ref.bit_rows(bits)
    return frozen(hashed, rows)


@functools.lru_cache(maxsize=None)
def bit_cvs(R, n, seed=0, base=0, root_ok=True):
    return frozen(b3_ref.chunk_cvs(bit_case(R, n, seed)[0], base, root_ok))


@functools.lru_cache(maxsize=None)
def word_case(R, n_words, seed=0):
    return frozen(np.random.default_rng([3, R, n_words, seed]).integers(0, 256, (R, 8 * n_words), dtype=np.uint8))


@functools.lru_cache(maxsize=None)
def word_cvs(R, n_words, seed=0, base=0, root_ok=True):
    return frozen(b3_ref.chunk_cvs(word_case(R, n_words, seed), base, root_ok))


@functools.lru_cache(maxsize=None)
def node_case(n, R, seed=0):
    """random chaining values [n, R, 8]"""
    return frozen(np.random.default_rng([4, n, R, seed]).integers(0, 2**32, (n, R, 8), dtype=np.uint32))


@functools.lru_cache(maxsize=None)
def node_root(n, R, seed=0):
    return frozen(b3_ref.tree(node_case(n, R, seed)))


def quad_lists(NQ):
    """ascending lists, as the verifier makes them, of 1, NQ/4, NQ/4 + 1, NQ - 1 and NQ quad words; each longer than one holds quad 0
    and quad NQ - 1"""
    out = [[0], [NQ - 1]]
    rng = np.random.default_rng(700 + NQ)
    for k in sorted({NQ // 4, NQ // 4 + 1, NQ - 1, NQ} - {0, 1}):
        mid = np.sort(rng.permutation(np.arange(1, NQ - 1))[:k - 2]).tolist()
        out.append([0] + mid + [NQ - 1])
    return out


def listed_reps(quads):
    return np.asarray([4 * q + i for q in quads for i in range(4)])


# ---- the hooks ----
def chunks_rc(hooks, kind, stream, n, width, R, stride=0, quads=None, n_quads=None, base=0, root_ok=1, choice=0, batch=0, cv_words=None):
    """-> (status, cvs [B][n_chunks][R][8], kernel launched); the words behind the chaining values are checked here"""
    L, h = hooks
    B = max(batch, 1)
    nc = b3_ref.n_chunks(8 * n if kind == 2 else n)
    words = nc * R * 8 + PAD if cv_words is None else cv_words
    out = np.zeros((B, max(words, 1)), np.uint32)
    chosen = C.c_uint32(99)
    q = None if quads is None else np.ascontiguousarray(quads, np.uint32)
    nq = (0 if q is None else len(q)) if n_quads is None else n_quads
    stream = np.ascontiguousarray(stream)
    rc = L.rv_hook_b3_chunks(h, kind, _p(stream), n, width, stride, _p(q), nq, base, root_ok, choice, batch, _p(out), words, C.byref(chosen))
    if rc:
        return rc, None, None
    assert (out[:, nc * R * 8:] == FILL32).all(), "words behind the last chaining value were written"
    return 0, out[:, :nc * R * 8].reshape(B, nc, R, 8), chosen.value


def chunks(hooks, *a, **k):
    rc, cvs, chosen = chunks_rc(hooks, *a, **k)
    assert rc == 0, rc
    return cvs, chosen


def tree_rc(hooks, cvs, R, choice=0, batch=0):
    """cvs [n, R, 8] or [B, n, R, 8] -> (status, digests [B][R][8], (reductions, nodes at the top, top kernel))"""
    L, h = hooks
    cvs = np.ascontiguousarray(cvs, np.uint32)
    B = max(batch, 1)
    n = cvs.shape[-3]
    out = np.zeros((B, R * 8 + PAD), np.uint32)
    plan = (C.c_uint32 * 3)()
    rc = L.rv_hook_b3_tree(h, _p(cvs), n, R, choice, batch, _p(out), R * 8 + PAD, plan)
    if rc:
        return rc, None, None
    assert (out[:, R * 8:] == FILL32).all(), "words behind the last digest were written"
    return 0, out[:, :R * 8].reshape(B, R, 8), tuple(plan)


def tree(hooks, *a, **k):
    rc, dig, plan = tree_rc(hooks, *a, **k)
    assert rc == 0, rc
    return dig, plan


def pair_small_rc(hooks, pre_rows, n_pre, on_rows, n_on, NQ, quads=None, n_quads=None, choice=0, batch=0):
    """-> (status, form taken, cv_pre [B][c_pre][R][8], cv_on, dig_pre [B][R][8], dig_on)"""
    L, h = hooks
    B, R = max(batch, 1), 4 * NQ
    wa, wb, wd = b3_ref.n_chunks(n_pre) * R * 8, b3_ref.n_chunks(n_on) * R * 8, R * 8
    cva, cvb = np.zeros((B, wa + PAD), np.uint32), np.zeros((B, wb + PAD), np.uint32)
    da, db = np.zeros((B, wd + PAD), np.uint32), np.zeros((B, wd + PAD), np.uint32)
    taken = C.c_uint32(99)
    q = None if quads is None else np.ascontiguousarray(quads, np.uint32)
    nq = (0 if q is None else len(q)) if n_quads is None else n_quads
    pre_rows, on_rows = np.ascontiguousarray(pre_rows), np.ascontiguousarray(on_rows)
    rc = L.rv_hook_b3_pair_small(h, _p(pre_rows), n_pre, _p(on_rows), n_on, NQ, _p(q), nq, choice, batch, _p(cva), wa + PAD, _p(cvb), wb + PAD, _p(da), _p(db),
                                 wd + PAD, C.byref(taken))
    if rc:
        return (rc,) + (None,) * 5
    for buf, w in ((cva, wa), (cvb, wb), (da, wd), (db, wd)):
        assert (buf[:, w:] == FILL32).all(), "words behind an output were written"
    return (0, taken.value, cva[:, :wa].reshape(B, -1, R, 8), cvb[:, :wb].reshape(B, -1, R, 8), da[:, :wd].reshape(B, R, 8), db[:, :wd].reshape(B, R, 8))


# ---- chunk kernels ----
def byte_choices(NQ):
    return [0, RPL1, RPL4] + ([UNI] if NQ == 64 else [])


@pytest.mark.parametrize("NQ", [64, 8, 2, 16, 32])
def test_byte_row_chunks(hooks, NQ):
    """k_b3_chunks<1>, k_b3_chunks<4>, k_b3_chunks_uni (full rows) and production's own pick (a repetition per lane at these sizes)"""
    R = 4 * NQ
    for n in COUNTS if NQ in (64, 8) else FEW:
        rows, want = byte_case(R, n)[1], byte_cvs(R, n)
        for choice in byte_choices(NQ):
            got, chosen = chunks(hooks, 0, rows, n, NQ, R, choice=choice)
            assert chosen == (choice or RPL1)
            same(got[0], want, f"byte rows NQ={NQ} events={n} kernel={chosen}")


@pytest.mark.parametrize("NQ", [64, 8, 2, 16, 32])
def test_bit_row_chunks(hooks, NQ):
    """k_b3_chunks_bits1, k_b3_chunks_bits, k_b3_chunks_bits_uni (full rows)"""
    R = 4 * NQ
    for n in COUNTS if NQ in (64, 8) else FEW:
        rows, want = bit_case(R, n)[1], bit_cvs(R, n)
        for choice in byte_choices(NQ):
            got, chosen = chunks(hooks, 1, rows, n, NQ, R, choice=choice)
            assert chosen == (choice or RPL1)
            same(got[0], want, f"bit rows NQ={NQ} events={n} kernel={chosen}")


@pytest.mark.parametrize("R", [8, 256])
def test_contig_chunks(hooks, R):
    """k_b3_chunks_contig: whole and partial blocks and words, the two-blocks-a-step path of full chunks, streams a stride apart"""
    for n in [0, 1, 7, 8, 9, 127, 128, 129, 255, 256, 257, 1000]:
        data, want = word_case(R, n), word_cvs(R, n)
        for stride in sorted({n, n + 3, 2048}):
            got, _ = chunks(hooks, 2, b3_ref.contig_streams(data, stride), n, R, R, stride=stride)
            same(got[0], want, f"contiguous R={R} words={n} stride={stride}")


def counter_cases(kind):
    """(rows, n, width, R, reference function) with three chunks, so that the second crosses into the counter's high word"""
    if kind == 0:
        return [(byte_case(4 * NQ, 2049)[1], 2049, NQ, 4 * NQ, functools.partial(byte_cvs, 4 * NQ, 2049, 0)) for NQ in (8, 64)]
    if kind == 1:
        return [(bit_case(4 * NQ, 2049)[1], 2049, NQ, 4 * NQ, functools.partial(bit_cvs, 4 * NQ, 2049, 0)) for NQ in (8, 64)]
    return [(b3_ref.contig_streams(word_case(R, 257), 260), 257, R, R, functools.partial(word_cvs, R, 257, 0)) for R in (8, 256)]


@pytest.mark.parametrize("kind", [0, 1, 2])
def test_chunk_counter(hooks, kind):
    """chunk_base: the chunk counter is 64 bits wide in every kernel (base + chunk crosses 2^32; a base above 2^40)"""
    for rows, n, width, R, ref in counter_cases(kind):
        for base in BASES:
            want = ref(base, True)
            for choice in ([0] if kind == 2 else byte_choices(width)):
                got, chosen = chunks(hooks, kind, rows, n, width, R, stride=260 if kind == 2 else 0, base=base, choice=choice)
                same(got[0], want, f"kind={kind} width={width} base={base} kernel={chosen}")


@pytest.mark.parametrize("kind", [0, 1, 2])
def test_lone_chunk_root(hooks, kind):
    """a lone chunk is the root only when the caller says so: root_ok = 0 leaves an ordinary leaf, at base 0 and above"""
    n = 13 if kind == 2 else 100
    for width in ((8, 256) if kind == 2 else (8, 64)):
        R = width if kind == 2 else 4 * width
        rows = b3_ref.contig_streams(word_case(R, n), n) if kind == 2 else (byte_case, bit_case)[kind](R, n)[1]
        ref = functools.partial((byte_cvs, bit_cvs, word_cvs)[kind], R, n, 0)
        for choice in ([0] if kind == 2 else byte_choices(width)):
            for base in (0, 5, 2**32):
                root, _ = chunks(hooks, kind, rows, n, width, R, stride=n if kind == 2 else 0, base=base, root_ok=1, choice=choice)
                leaf, _ = chunks(hooks, kind, rows, n, width, R, stride=n if kind == 2 else 0, base=base, root_ok=0, choice=choice)
                same(root[0], ref(base, True), f"kind={kind} width={width} base={base} root_ok=1 choice={choice}")
                same(leaf[0], ref(base, False), f"kind={kind} width={width} base={base} root_ok=0 choice={choice}")
                assert not (root == leaf).all(axis=-1).any()


@pytest.mark.parametrize("NQ", [8, 16, 64])
def test_byte_row_quad_lists(hooks, NQ):
    """the verifier's quad list: the listed quad words' repetitions get their chaining values, every other word stays 0xA5"""
    R = 4 * NQ
    for n in [0, 65, 1025, 2049]:
        rows, want = byte_case(R, n)[1], byte_cvs(R, n)
        for quads in quad_lists(NQ):
            for choice in (0, RPL1, RPL4):
                got, chosen = chunks(hooks, 0, rows, n, NQ, R, quads=quads, choice=choice)
                assert chosen == (choice or RPL1)
                same(got[0], b3_ref.scatter_quads(want, quads), f"byte rows NQ={NQ} events={n} quads={len(quads)} kernel={chosen}")


@pytest.mark.parametrize("kind", [0, 1, 2])
def test_chunks_batched(hooks, kind):
    """eight different streams recorded and replayed as one batch (k_many): every chunk kernel's body, each output against its input"""
    B, NQ, R = 8, 64, 256
    for n in (9, 129, 509) if kind == 2 else (65, 1025, 4072):
        if kind == 2:
            rows = np.stack([b3_ref.contig_streams(word_case(R, n, b), n + 1) for b in range(B)])
            want = np.stack([word_cvs(R, n, b) for b in range(B)])
        else:
            case, cvs = (byte_case, byte_cvs) if kind == 0 else (bit_case, bit_cvs)
            rows = np.stack([case(R, n, b)[1] for b in range(B)])
            want = np.stack([cvs(R, n, b) for b in range(B)])
        for choice in ([0] if kind == 2 else byte_choices(NQ)):
            got, chosen = chunks(hooks, kind, rows, n, R if kind == 2 else NQ, R, stride=n + 1 if kind == 2 else 0, choice=choice, batch=B)
            same(got, want, f"batch of {B}: kind={kind} n={n} kernel={chosen}")


# ---- paired chunk kernels ----
MIXED = [(0, 0), (1, 4072), (4072, 1), (1024, 1025), (65536, 64), (64, 65536)]  # the last two: 64 chunks beside one, the most the pair takes


def check_pair_small(hooks, NQ, n_pre, n_on, choice, quads=None, seed=0):
    R = 4 * NQ
    rc, taken, cva, cvb, da, db = pair_small_rc(hooks, bit_case(R, n_pre, seed)[1], n_pre, byte_case(R, n_on, seed)[1], n_on, NQ, quads=quads, choice=choice)
    what = f"small pair NQ={NQ} events=({n_pre}, {n_on}) form={taken} quads={None if quads is None else len(quads)}"
    assert rc == 0 and taken == (choice or PAIR_Q), what
    want_a, want_b = bit_cvs(R, n_pre, seed), byte_cvs(R, n_on, seed)
    same(cva[0], want_a, what + " preprocessing chaining values")
    same(da[0], b3_ref.tree(want_a), what + " preprocessing digests")
    if quads is None:
        same(cvb[0], want_b, what + " online chaining values")
        same(db[0], b3_ref.tree(want_b), what + " online digests")
    else:  # (the tree above skipped quad words runs on whatever the buffer held: only the listed repetitions' digests mean anything)
        same(cvb[0], b3_ref.scatter_quads(want_b, quads), what + " online chaining values")
        reps = listed_reps(quads)
        same(db[0][reps], b3_ref.tree(want_b)[reps], what + " online digests of the listed repetitions")


@pytest.mark.parametrize("choice", [0, PAIR_Q, PAIR_LANE])
@pytest.mark.parametrize("NQ", [8, 64])
def test_pair_small(hooks, NQ, choice):
    """k_b3_chunks_pair_q (production's pick for one proof) and k_b3_chunks_pair, then k_b3_tree_tail_pair: both streams' chaining values
    and digests, at every count and at the quad-of-lanes kernel's column edges"""
    counts = COUNTS + QCOLS
    for n_pre, n_on in MIXED + list(zip(counts, counts[::-1])):
        check_pair_small(hooks, NQ, n_pre, n_on, choice)


@pytest.mark.parametrize("choice", [0, PAIR_Q, PAIR_LANE])
@pytest.mark.parametrize("NQ", [8, 64])
def test_pair_small_quad_lists(hooks, NQ, choice):
    for n_pre, n_on in [(0, 0), (65, 1025), (1025, 49), (17, 4072)]:
        for quads in quad_lists(NQ):
            check_pair_small(hooks, NQ, n_pre, n_on, choice, quads=quads)


def test_pair_small_tree_tops(hooks):
    """k_b3_tree_tail_pair at every node count that changes its walk, different in the two streams"""
    NQ = 8
    tops = list(range(1, 10)) + [15, 16, 17, 31, 32, 33, 63, 64]
    for c_pre, c_on in zip(tops, tops[::-1]):
        check_pair_small(hooks, NQ, 1024 * c_pre - 5, 1024 * (c_on - 1) + 1, 0)


def test_pair_small_declines_and_batch(hooks):
    NQ, R = 64, 256
    # more than 64 chunks in a stream, or a list without quad words: nothing is launched, every buffer comes back as it went
    for n_pre, n_on, quads, nq in [(64 * 1024 + 1, 1, None, None), (1, 64 * 1024 + 1, None, None), (65, 65, [0], 0)]:
        rc, taken, cva, cvb, da, db = pair_small_rc(hooks, bit_case(R, n_pre)[1], n_pre, byte_case(R, n_on)[1], n_on, NQ, quads=quads, n_quads=nq)
        assert rc == 0 and taken == 0
        assert all((x == FILL32).all() for x in (cva, cvb, da, db))
    # a batch of eight: the lane form, each proof's four outputs against its own two inputs
    B = 8
    for n_pre, n_on in [(1025, 65), (4072, 4072)]:
        pre, on = np.stack([bit_case(R, n_pre, b)[1] for b in range(B)]), np.stack([byte_case(R, n_on, b)[1] for b in range(B)])
        for choice in (0, PAIR_LANE):
            rc, taken, cva, cvb, da, db = pair_small_rc(hooks, pre, n_pre, on, n_on, NQ, choice=choice, batch=B)
            assert rc == 0 and taken == PAIR_LANE
            for b in range(B):
                same(cva[b], bit_cvs(R, n_pre, b), f"batched small pair {b}: preprocessing chaining values")
                same(cvb[b], byte_cvs(R, n_on, b), f"batched small pair {b}: online chaining values")
                same(da[b], b3_ref.tree(bit_cvs(R, n_pre, b)), f"batched small pair {b}: preprocessing digests")
                same(db[b], b3_ref.tree(byte_cvs(R, n_on, b)), f"batched small pair {b}: online digests")


def test_pair_big_chunks(hooks):
    """k_b3_chunks_pair_uni<0|1|2>: no list, a list of more than a quarter of the row (a lane per quad word), a quarter or less (a lane
    per repetition) -- the shared launch's block split between the two streams at a few chunks"""
    L, h = hooks
    NQ, R = 64, 256
    for n_pre, n_on in [(1, 1), (1025, 3000), (3000, 1025)]:
        want_a, want_b = bit_cvs(R, n_pre), byte_cvs(R, n_on)
        for quads in [None] + quad_lists(NQ):
            cva, cvb = np.zeros(want_a.size + PAD, np.uint32), np.zeros(want_b.size + PAD, np.uint32)
            q = None if quads is None else np.asarray(quads, np.uint32)
            rc = L.rv_hook_b3_pair_big_chunks(h, _p(bit_case(R, n_pre)[1]), n_pre, _p(byte_case(R, n_on)[1]), n_on, _p(q), 0 if q is None else len(q), _p(cva),
                                              len(cva), _p(cvb), len(cvb))
            what = f"big pair events=({n_pre}, {n_on}) quads={None if quads is None else len(quads)}"
            assert rc == 0, what
            assert (cva[want_a.size:] == FILL32).all() and (cvb[want_b.size:] == FILL32).all(), what
            same(cva[:want_a.size].reshape(want_a.shape), want_a, what + " preprocessing")
            same(cvb[:want_b.size].reshape(want_b.shape), want_b if quads is None else b3_ref.scatter_quads(want_b, quads), what + " online")


# ---- trees ----
SMALL_TOPS = list(range(1, 10)) + [15, 16, 17, 31, 32, 33, 63, 64]
BIG_TOPS = [65, 127, 128, 129, 255, 256, 257, 511, 512]


@pytest.mark.parametrize("top", [LANE, TAIL64, TAIL512])
def test_tree_tops(hooks, top):
    """k_b3_tree_lane (every n up to 64: its binary counter has a case per bit pattern), k_b3_tree_tail_small, k_b3_tree_tail; one node
    is copied (the chunk kernel applied ROOT)"""
    R = 8
    for n in {LANE: list(range(1, 65)), TAIL64: SMALL_TOPS, TAIL512: SMALL_TOPS + BIG_TOPS}[top]:
        got, plan = tree(hooks, node_case(n, R), R, choice=top)
        assert plan == (0, n, top)
        same(got[0], node_root(n, R), f"tree top {top} n={n}")
        if n == 1:
            same(got[0], node_case(1, R)[0], "one node is its own root")
    for R in (64, 256):  # one wavefront and four of them (8: part of one)
        for n in (3, 64):
            got, _ = tree(hooks, node_case(n, R), R, choice=top)
            same(got[0], node_root(n, R), f"tree top {top} n={n} R={R}")


def test_tree_natural_pick(hooks):
    R = 8
    for n in SMALL_TOPS + BIG_TOPS:
        got, plan = tree(hooks, node_case(n, R), R)
        assert plan == (0, n, LANE if n <= 4 else TAIL64 if n <= 64 else TAIL512)
        same(got[0], node_root(n, R), f"tree n={n}")


def test_tree_reductions(hooks):
    """one, two and three k_b3_reduce<2> launches; a ragged last group of every size, also in the second launch (2 053 -> 514 -> 129)"""
    for n, reduces, R in [(513, 1, 8), (514, 1, 8), (515, 1, 8), (516, 1, 8), (517, 1, 8), (2047, 1, 8), (2048, 1, 8), (2049, 2, 8), (2050, 2, 8), (2053, 2, 8),
                          (8193, 3, 8), (513, 1, 256), (2049, 2, 256)]:
        got, plan = tree(hooks, node_case(n, R), R)
        assert plan[0] == reduces and plan[2] == TAIL512
        same(got[0], node_root(n, R), f"tree n={n} R={R} ({reduces} reductions, {plan[1]} nodes at the top)")


def test_tree_batched(hooks):
    """a batch of eight trees: production's pick (a lane per repetition up to 64 nodes) and every top through k_many"""
    B, R = 8, 8
    for n in (1, 5, 64, 65, 513):
        cvs = np.stack([node_case(n, R, b) for b in range(B)])
        want = np.stack([node_root(n, R, b) for b in range(B)])
        got, plan = tree(hooks, cvs, R, batch=B)
        assert plan[2] == (LANE if n <= 64 else TAIL512) and plan[0] == (1 if n == 513 else 0)
        same(got, want, f"batch of {B} trees n={n}")
        for top in ([TAIL64] if n <= 64 else []) + [TAIL512]:
            got, plan = tree(hooks, cvs, R, choice=top, batch=B)
            assert plan[2] == top
            same(got, want, f"batch of {B} trees n={n} top={top}")


def pair_big_tree(hooks, n_a, n_b, R):
    L, h = hooks
    da, db = np.zeros(R * 8 + PAD, np.uint32), np.zeros(R * 8 + PAD, np.uint32)
    launches = C.c_uint32(0)
    rc = L.rv_hook_b3_pair_big_tree(h, _p(node_case(n_a, R, 1)), n_a, _p(node_case(n_b, R, 2)), n_b, R, _p(da), _p(db), R * 8 + PAD, C.byref(launches))
    assert rc == 0, rc
    assert (da[R * 8:] == FILL32).all() and (db[R * 8:] == FILL32).all()
    return da[:R * 8].reshape(R, 8), db[:R * 8].reshape(R, 8), launches.value


def test_pair_big_tree(hooks):
    """k_b3_reduce_pair (three levels a launch) and k_b3_tree_tail_pair_big (up to 1 024 nodes, 512 threads): both streams reduced, one
    sitting a launch out -- it must come out right from whichever ping-pong buffer it ended in --, config 4's own shape"""
    cases = [(65, 65, 8), (1024, 1024, 8), (1025, 65, 8), (65, 1025, 8), (1025, 1024, 8), (1031, 1025, 8), (8192, 1025, 8), (8193, 8200, 8), (8200, 65, 8),
             (613 * 8 - 4, 1025, 8), (1025, 613, 256)]
    for n_a, n_b, R in cases:
        want_launches = 1
        a, b = n_a, n_b
        while a > 1024 or b > 1024:
            a, b = (a + 7) // 8 if a > 1024 else a, (b + 7) // 8 if b > 1024 else b
            want_launches += 1
        da, db, launches = pair_big_tree(hooks, n_a, n_b, R)
        assert launches == want_launches
        same(da, node_root(n_a, R, 1), f"big pair tree ({n_a}, {n_b}) R={R}: first stream")
        same(db, node_root(n_b, R, 2), f"big pair tree ({n_a}, {n_b}) R={R}: second stream")


def piece_lists(n):
    """how n - 1 chaining values arrive: one at a time, all at once, in doubling pieces, in pieces from a fixed seed with empty ones"""
    m = n - 1
    out = [[1] * m, [m]]
    dbl, k = [], 1
    while sum(dbl) < m:
        dbl.append(min(k, m - sum(dbl)))
        k *= 2
    out.append(dbl)
    rng = np.random.default_rng(900 + n)
    rnd = []
    while sum(rnd) < m:
        rnd.append(int(min(rng.integers(0, 8), m - sum(rnd))))
    out.append(rnd + [0])
    return out


@pytest.mark.parametrize("R", [8, 256])
@pytest.mark.parametrize("B", [1, 2, 33])
def test_incremental_tree(hooks, B, R):
    """inc_absorb / inc_finish (k_b3_pairs for one stream, k_b3_pairs_batched for several -- 33: two launches a level --, k_b3_fold):
    the tree over all values however they were cut"""
    L, h = hooks
    for n in [1, 2, 3, 4, 5, 8, 9, 31, 32, 33, 100]:
        cvs = node_case(n, B * R, 5).reshape(n, B, R, 8).transpose(1, 0, 2, 3)  # [B][n][R][8]
        dev = np.ascontiguousarray(cvs)
        want = b3_ref.incremental(node_case(n, B * R, 5), piece_lists(n)[0]).reshape(B, R, 8)  # (the same for every cut)
        for pieces in piece_lists(n):
            assert sum(pieces) == n - 1
            out = np.zeros((B, R * 8 + PAD), np.uint32)
            pc = np.asarray(pieces, np.uint64)
            rc = L.rv_hook_b3_incremental(h, _p(dev), n, R, B, _p(pc) if len(pc) else None, len(pc), _p(out), R * 8 + PAD)
            assert rc == 0, rc
            assert (out[:, R * 8:] == FILL32).all()
            same(out[:, :R * 8].reshape(B, R, 8), want, f"incremental tree n={n} B={B} R={R} pieces={pieces[:12]}")


@pytest.mark.parametrize("R", [8, 64, 72, 256])
def test_join(hooks, R):
    """k_join: h = B3(B3(pre2 || on2) || B3(pre64 || on64)); digests behind repetition R - 1 stay untouched (72: a partial wavefront)"""
    L, h = hooks
    for batch in (0, 8):
        B = max(batch, 1)
        digs = np.random.default_rng([6, R, batch]).integers(0, 2**32, (B, 4, R, 8), dtype=np.uint32)
        out = np.zeros((B, R * 32 + 4 * PAD), np.uint8)
        rc = L.rv_hook_b3_join(h, _p(digs), R, batch, _p(out), out.shape[1])
        assert rc == 0, rc
        assert (out[:, R * 32:] == 0xA5).all()
        for b in range(B):
            same(out[b, :R * 32].reshape(R, 32), b3_ref.join(*digs[b]), f"join R={R} batch={batch} proof {b}")


# ---- end to end through the split launchers ----
@pytest.mark.parametrize("kind", [0, 1, 2])
def test_end_to_end_vs_official(hooks, kind):
    """chunk launch + tree launch, production's own picks, against the official BLAKE3 of each repetition's byte string: this ties the
    layout helpers of tests/b3_ref.py to something outside it"""
    official = b3_ref.load_official()
    NQ, R = 64, 256
    if kind == 2:
        n, data = 509, word_case(R, 509)
        rows = b3_ref.contig_streams(data, 512)
    else:
        n = 4072
        data, rows = (byte_case, bit_case)[kind](R, n)
    cvs, _ = chunks(hooks, kind, rows, n, R if kind == 2 else NQ, R, stride=512 if kind == 2 else 0)
    dig, _ = tree(hooks, cvs[0], R)
    got = b3_ref.digest_bytes(dig[0])
    for r in range(R):
        assert got[r].tobytes() == official(data[r].tobytes()), (kind, r)


# ---- what the hooks refuse (before anything is launched) ----
def test_refusals(hooks):
    L, h = hooks
    rows8, rows64 = byte_case(32, 65)[1], byte_case(256, 65)[1]
    bits8 = bit_case(32, 65)[1]
    rc = lambda *a, **k: chunks_rc(hooks, *a, **k)[0]  # noqa: E731
    assert rc(0, rows8, 65, 8, 32, choice=UNI) == E_ARG                          # a chunk per wavefront needs rows of 64 quad words
    assert rc(1, bits8, 65, 8, 32, choice=UNI) == E_ARG
    assert rc(0, rows64, 65, 64, 256, quads=[0, 5], choice=UNI) == E_ARG         # ... and no quad list
    assert rc(1, bits8, 65, 7, 28) == E_ARG                                      # bit rows hold two quad words a byte
    assert rc(1, bits8, 65, 8, 32, quads=[0]) == E_ARG                           # ... and take no list
    assert rc(0, rows8, 65, 8, 32, quads=[3, 2]) == E_ARG                        # not ascending
    assert rc(0, rows8, 65, 8, 32, quads=[2, 2]) == E_ARG
    assert rc(0, rows8, 65, 8, 32, quads=[0, 8]) == E_ARG                        # past the row
    assert rc(0, rows8, 65, 8, 32, quads=[0], n_quads=0) == E_ARG                # a list without quad words: production launches nothing
    assert rc(0, rows8, 65, 8, 32, cv_words=32 * 8 - 1) == E_ARG                 # an output that does not hold the chaining values
    assert rc(0, rows8, 65, 8, 32, batch=1) == E_ARG
    assert rc(0, rows8, 65, 8, 32, choice=4) == E_ARG
    words = b3_ref.contig_streams(word_case(8, 9), 9)
    assert rc(2, words, 9, 8, 8, stride=8) == E_ARG                              # streams that overlap
    assert rc(2, words, 9, 8, 8, stride=9, choice=RPL1) == E_ARG                 # one kernel: nothing to force
    for top, n in [(LANE, 65), (TAIL64, 65), (LANE, 513), (TAIL64, 2049)]:       # 513 -> 129, 2 049 -> 129 nodes at the top
        assert tree_rc(hooks, node_case(n, 8), 8, choice=top)[0] == E_ARG
    assert tree_rc(hooks, node_case(5, 8), 8, choice=4)[0] == E_ARG
    pre, on = bit_case(256, 64 * 1024 + 1)[1], byte_case(256, 1)[1]
    assert pair_small_rc(hooks, pre, 64 * 1024 + 1, on, 1, 64, choice=PAIR_Q)[0] == E_ARG      # 65 chunks: past the 64-node top
    assert pair_small_rc(hooks, pre, 64 * 1024 + 1, on, 1, 64, choice=PAIR_LANE)[0] == E_ARG
    pre8 = np.stack([bit_case(32, 65, b)[1] for b in range(2)])
    on8 = np.stack([byte_case(32, 65, b)[1] for b in range(2)])
    assert pair_small_rc(hooks, pre8, 65, on8, 65, 8, choice=PAIR_Q, batch=2)[0] == E_ARG       # the quad-of-lanes form is not recorded
    assert pair_small_rc(hooks, pre8, 65, on8, 65, 7)[0] == E_ARG
    out = np.zeros(8 * 8 + PAD, np.uint32)
    cv = node_case(5, 8)
    assert L.rv_hook_b3_incremental(h, _p(cv), 5, 8, 1, _p(np.asarray([1, 2], np.uint64)), 2, _p(out), len(out)) == E_ARG   # pieces must sum to n - 1
    assert L.rv_hook_b3_incremental(h, _p(cv), 5, 8, 1, _p(np.asarray([5], np.uint64)), 1, _p(out), len(out)) == E_ARG
    assert L.rv_hook_b3_join(h, _p(node_case(4, 8)), 8, 0, _p(np.zeros(255, np.uint8)), 255) == E_ARG
