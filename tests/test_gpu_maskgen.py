"""Every AES-128-CTR mask generator, as a shard launches it, against tests/maskgen_ref.py -- bit for bit, at every width that picks
another kernel instantiation or quad-group count, across the counter-byte carries (block 255 -> 256, 65 535 -> 65 536), up to the last
legal counter 2^24 - 1, with and without keep words, and through both key setups (the three launches and the fused k_setup_keys).

rv_hook_maskgen returns the device rows untouched; the reference builds them from the oracle's keystream and the definition of the
layout (tests/test_maskgen_ref_host.py ties it to the oracle's share generators and the golden shares).  Not reached from here:
k_z64_fused, which runs the same first rounds inside another kernel and has no launch without a gate list.  Its cipher is pinned at the
same windows, and at every carry into counter bits 16..23, by tests/test_gpu_z64_fused_level.py (rv_hook_z64_fused_run: Mul and Input
levels at any first_block, against tests/z64f_ref.py, which takes its fresh masks from this file's reference)."""
import ctypes as C
import functools

import numpy as np
import pytest

import maskgen_ref

pytestmark = pytest.mark.gpu

GENERATORS = {0: "k_aes_gf2_masks", 1: "k_aes_gf2_masks_col4", 2: "k_aes_z64_masks"}
KEY_PATHS = {0: "expand_seeds + key_schedule + bitslice_rk (+ rk_col4)", 1: "k_setup_keys"}
# R -> (NQ, quad words per workgroup, quad groups): one width per instantiation and per quad-group count
WIDTHS_PLANES = [8, 24, 32, 96, 64, 256]  # QW 2 x 1, 2 x 3, 8 x 1, 8 x 3, 16 x 1, 16 x 4 (production)
WIDTHS_COL4 = [64, 192, 256]              # 1, 3, 4 groups of 16 quad words
BOTH_KEY_PATHS = (64, 256)
MAX_CTR = 1 << 24
WINDOWS = [
    (0, 1),
    (0, 33),               # at NQ = 64 two chunks of the 128-plane kernel, the second a single block beside idle lanes
    (250, 12),             # counter byte 15 carries into byte 14
    (65530, 12),           # bytes 14 and 15 wrap, byte 13 becomes 1
    (MAX_CTR - 12, 12),    # ends on the last legal counter
]
MULTI_CHUNK = (65536 - 129, 257)  # several chunks per quad group and a tail, at both ends of the quad-group count
MULTI_CHUNK_WIDTHS = (8, 256)
OMITS = ["null", "none", "mixed"]


def _cases():
    out = []
    for gen, widths in ((0, WIDTHS_PLANES), (1, WIDTHS_COL4), (2, WIDTHS_PLANES)):
        for R in widths:
            for w in WINDOWS + ([MULTI_CHUNK] if R in MULTI_CHUNK_WIDTHS else []):
                out.append(pytest.param(gen, R, w, id=f"{GENERATORS[gen]}-R{R}-{w[0]}+{w[1]}"))
    return out


def _seeds(R):
    return np.random.default_rng(9000 + R).integers(0, 256, (R, 16), dtype=np.uint8)


def _omits(R, kind):
    """the omit vectors of one kind: None (the prover's launch, no keep words), all 8, or a fixed-seed mix of players and 8 in which
    every player occurs (R = 8 has no room for all eight players AND an 8: a permutation of the players, then one with 8s in it)"""
    if kind == "null":
        return [None]
    if kind == "none":
        return [np.full(R, 8, np.uint8)]
    rng = np.random.default_rng(77 + R)
    if R >= 16:
        v = np.concatenate([np.arange(9), rng.integers(0, 9, R - 9)]).astype(np.uint8)
        rng.shuffle(v)
        assert set(v.tolist()) == set(range(9))
        return [v]
    perm = rng.permutation(8).astype(np.uint8)
    some = perm.copy()
    some[rng.permutation(8)[:3]] = 8
    return [perm, some]


@functools.lru_cache(maxsize=None)
def _reference(R, window, kind, domain):
    """the expected rows of every omit vector of `kind`: computed once per (seeds, window, omit), shared by the generators and key paths"""
    out = []
    for omit in _omits(R, kind):
        ks = _keystream(R, window, kind, 0 if omit is None else omit.tobytes())
        rows = maskgen_ref.z64_rows(ks) if domain == 64 else maskgen_ref.gf2_rows(ks)
        rows.setflags(write=False)
        out.append(rows)
    return out


@functools.lru_cache(maxsize=8)
def _keystream(R, window, kind, omit_key):
    omit = None if omit_key == 0 else np.frombuffer(omit_key, np.uint8)
    return maskgen_ref.keystream(_seeds(R), omit, window[0], window[1])


@pytest.fixture(scope="module")
def hook(oracle):
    import reverie_amd
    from reverie_amd import _lib

    ctx = reverie_amd.Context.default()  # raises loudly if the HIP library or the GPU is missing

    def call(seeds, omit, gen, key_path, first, n, out):
        seeds = np.ascontiguousarray(seeds, dtype=np.uint8)
        return _lib.lib().rv_hook_maskgen(ctx.handle, seeds.ctypes.data_as(C.c_void_p), seeds.shape[0],
                                          None if omit is None else omit.ctypes.data_as(C.c_void_p), gen, key_path, first, n,
                                          out.ctypes.data_as(C.c_void_p))

    return call


def _empty_rows(gen, R, n):
    # (a pattern no keystream is expected to produce in every word: a row the launch skipped stays visible)
    if gen == 2:
        return np.full((2 * n, 8 * R), 0xA5A5A5A5A5A5A5A5, np.uint64)
    return np.full((128 * n, R // 4), 0xA5A5A5A5, np.uint32)


@pytest.mark.parametrize("gen,R,window", _cases())
def test_maskgen(hook, gen, R, window):
    first, n = window
    seeds = _seeds(R)
    for kind in OMITS:
        wants = _reference(R, window, kind, 64 if gen == 2 else 2)
        for omit, want in zip(_omits(R, kind), wants):
            rows = {}
            for kp in (0, 1) if R in BOTH_KEY_PATHS else (0,):
                got = _empty_rows(gen, R, n)
                assert got.shape == want.shape and got.dtype == want.dtype
                rc = hook(seeds, omit, gen, kp, first, n, got)
                where = (f"generator {gen} ({GENERATORS[gen]}), key path {kp} ({KEY_PATHS[kp]}), R = {R}, omit {kind}"
                         f"{'' if omit is None else ' ' + str(omit.tolist())}, blocks [{first}, {first + n})")
                assert rc == 0, f"{where}: error {rc}"
                if not np.array_equal(got, want):
                    diff = maskgen_ref.first_diff_z64 if gen == 2 else maskgen_ref.first_diff_gf2
                    pytest.fail(f"{where}: first difference at {diff(got, want, first)}")
                rows[kp] = got
            if len(rows) == 2:
                assert np.array_equal(rows[0], rows[1]), f"generator {gen}, R = {R}: the two key setups give different rows"


def test_col4_equals_planes(hook):
    """the two GF(2) generators write the same rows (one shard may take either: shard_setup_prg) -- directly, not only through the reference"""
    R, (first, n) = 256, (65530, 12)
    omit = _omits(R, "mixed")[0]
    a, b = _empty_rows(0, R, n), _empty_rows(1, R, n)
    assert hook(_seeds(R), omit, 0, 1, first, n, a) == 0 and hook(_seeds(R), omit, 1, 1, first, n, b) == 0
    assert np.array_equal(a, b), maskgen_ref.first_diff_gf2(b, a, first)


E_UNSUPPORTED, E_ARG = 8, 9


@pytest.mark.parametrize("gen,R,omit9,first,n,codes", [
    (1, 32, False, 0, 1, (E_UNSUPPORTED,)),                           # the lane-distributed generator takes whole groups of 16 quad words
    (0, 64, False, MAX_CTR - 11, 12, (E_UNSUPPORTED, E_ARG)),         # first_block + n_blocks = 2^24 + 1
    (1, 64, False, MAX_CTR - 11, 12, (E_UNSUPPORTED, E_ARG)),
    (2, 64, False, MAX_CTR, 1, (E_UNSUPPORTED, E_ARG)),
    (0, 64, False, 2**64 - 1, 2, (E_UNSUPPORTED, E_ARG)),             # (the sum wraps)
    (0, 12, False, 0, 1, (E_ARG, E_UNSUPPORTED)),                     # R is not a multiple of 8
    (2, 264, False, 0, 1, (E_ARG, E_UNSUPPORTED)),
    (0, 8, True, 0, 1, (E_ARG, E_UNSUPPORTED)),                       # an omit value above 8
    (3, 8, False, 0, 1, (E_ARG, E_UNSUPPORTED)),                      # no such generator
], ids=["col4-R32", "gf2-past-2^24", "col4-past-2^24", "z64-past-2^24", "window-wraps", "R12", "R264", "omit9", "generator3"])
def test_maskgen_rejects(hook, gen, R, omit9, first, n, codes):
    """host-side returns, before any launch: the output buffer is not touched"""
    seeds = np.zeros((R, 16), np.uint8)
    omit = np.full(R, 8, np.uint8)
    if omit9:
        omit[R - 1] = 9
    out = np.full(1 << 16, 0xA5A5A5A5, np.uint32)  # (larger than anything these arguments describe after wrapping)
    assert hook(seeds, omit, gen, 0, first, n, out) in codes
    assert (out == 0xA5A5A5A5).all()
    assert hook(seeds, None if not omit9 else omit, gen, 1, first, n, out) in codes
    assert (out == 0xA5A5A5A5).all()
