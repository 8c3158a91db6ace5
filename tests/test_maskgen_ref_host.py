"""The mask generators' numpy reference (tests/maskgen_ref.py) against the three independent pins the suite already has -- the
oracle's single-block PRG, its share generators, the committed golden shares -- before tests/test_gpu_maskgen.py compares any
GPU result with it.  Host only."""
import ctypes as C
import hashlib
import json
import os

import numpy as np
import pytest

import maskgen_ref
from conftest import GOLDEN

# the counter windows of tests/test_gpu_maskgen.py: byte 15 -> 14 carry, bytes 14 and 15 wrapping into 13, the last legal counter
WINDOWS = [(0, 5), (250, 12), (65530, 12), (2**24 - 12, 12), (65536 - 129, 257)]


def test_prg_blocks_equals_prg_block(oracle):
    rng = np.random.default_rng(21)
    keys = rng.integers(0, 256, (5, 16), dtype=np.uint8)
    keys[0] = 0
    blk = C.create_string_buffer(16)
    seen = set()
    for first, n in WINDOWS:
        out = oracle.prg_blocks(keys, first, n)
        assert out.shape == (5, n, 16)
        for k in range(5):
            for b in range(n):
                oracle.lib().rvo_prg_block(keys[k].tobytes(), C.c_uint64(first + b), blk)
                assert out[k, b].tobytes() == blk.raw, (k, first + b)
        seen.update(range(first, first + n))
    assert {255, 256, 65535, 65536, 2**24 - 1} <= seen


def test_prg_blocks_golden(oracle):
    prim = json.load(open(os.path.join(GOLDEN, "primitives.json")))
    keys = np.array([list(bytes.fromhex(v["key"])) for v in prim["aes_ctr"]], np.uint8)
    n = len(prim["aes_ctr"][0]["stream"]) // 32
    out = oracle.prg_blocks(keys, 0, n)
    for k, v in enumerate(prim["aes_ctr"]):
        assert out[k].tobytes().hex() == v["stream"]
    # a window that does not start at block 0 is the same stream
    assert (oracle.prg_blocks(keys, 2, n - 2) == out[:, 2:]).all()


def test_counter_is_big_endian_in_bytes_13_to_15(oracle):
    """The property the generators' first-round shortcut rests on, stated on the definition: block j < 2^24 encrypts the all-zero
    block with j in bytes 13..15, most significant first (FIPS-197 single-block encryption through the oracle's AES)."""
    key = np.arange(16, dtype=np.uint8)
    ctx = C.create_string_buffer(176)
    oracle.lib().rvo_aes128_init(ctx, key.tobytes())
    out = C.create_string_buffer(16)
    for j in (1, 255, 256, 65535, 65536, 0x123456, 2**24 - 1):
        pt = bytes(13) + bytes([j >> 16, (j >> 8) & 255, j & 255])
        oracle.lib().rvo_aes128_encrypt_portable(ctx, pt, out)
        assert oracle.prg_blocks(key, j, 1).tobytes() == out.raw, j


@pytest.mark.parametrize("seed", [5, 6])
def test_reference_equals_oracle_sharegen(oracle, seed):
    rng = np.random.default_rng(seed)
    seeds = rng.integers(0, 256, (8, 16), dtype=np.uint8)
    keys = np.stack([oracle.expand_seed(s) for s in seeds])
    for omit in (None, np.full(8, 8), rng.permutation(8), rng.integers(0, 9, 8)):
        om32 = np.full(8, 8, np.uint32) if omit is None else np.asarray(omit, np.uint32)
        ks = maskgen_ref.keystream(seeds, omit, 0, 40)
        assert (ks == maskgen_ref.keystream_from_keys(keys, omit, 0, 40)).all()
        rows = maskgen_ref.gf2_rows(ks)
        assert rows.dtype == np.uint32 and rows.shape == (40 * 128, 2)
        for n in (1, 127, 128, 129, 5000):
            assert (maskgen_ref.sharegen_gf2_layout(rows, n) == oracle.sharegen_gf2(keys, om32, n)).all()
        rows64 = maskgen_ref.z64_rows(ks)
        assert rows64.dtype == np.uint64 and rows64.shape == (80, 64)
        for n in (1, 2, 3, 79, 80):
            assert (maskgen_ref.sharegen_z64_layout(rows64, n) == oracle.sharegen_z64(keys, om32, n)).all()


def test_reference_equals_golden_sharegen(oracle):
    sg = json.load(open(os.path.join(GOLDEN, "sharegen.json")))
    keys = np.array([[list(bytes.fromhex(k)) for k in row] for row in sg["keys"]], np.uint8)
    n = sg["n"]
    for case in sg["cases"]:
        ks = maskgen_ref.keystream_from_keys(keys, case["omit"], 0, (n + 1) // 2)
        gf2 = maskgen_ref.sharegen_gf2_layout(maskgen_ref.gf2_rows(ks), n)
        assert ["%016x" % int(x) for x in gf2] == case["gf2"]
        z = maskgen_ref.sharegen_z64_layout(maskgen_ref.z64_rows(ks), n)
        zs = [["%016x" % int(v) for v in row.reshape(-1)] for row in z]
        assert zs[:4] == case["z64_first4"] and zs[-1] == case["z64_last"]
        assert hashlib.sha256(json.dumps(zs).encode()).hexdigest() == case["z64_sha256_json"]


def test_reference_wide_shard_is_its_groups_side_by_side(oracle):
    """A shard of R repetitions is R / 8 independent groups of 8: the wide rows are the groups' rows next to each other, in a
    window that does not start at block 0 and with a different omitted player per repetition."""
    rng = np.random.default_rng(7)
    R, first, n = 24, 65530, 12
    seeds = rng.integers(0, 256, (R, 16), dtype=np.uint8)
    omit = rng.integers(0, 9, R)
    ks = maskgen_ref.keystream(seeds, omit, first, n)
    rows, rows64 = maskgen_ref.gf2_rows(ks), maskgen_ref.z64_rows(ks)
    assert rows.shape == (n * 128, R // 4) and rows64.shape == (2 * n, 8 * R)
    for g in range(R // 8):
        ksg = maskgen_ref.keystream(seeds[8 * g:8 * g + 8], omit[8 * g:8 * g + 8], first, n)
        assert (rows[:, 2 * g:2 * g + 2] == maskgen_ref.gf2_rows(ksg)).all()
        assert (rows64[:, 64 * g:64 * g + 64] == maskgen_ref.z64_rows(ksg)).all()
    # ... and a window is a slice of the stream from block 0 (first + n blocks of one group would be too many here: a shifted pair)
    ks2 = maskgen_ref.keystream(seeds, omit, first + 5, n - 5)
    assert (maskgen_ref.gf2_rows(ks2) == rows[5 * 128:]).all() and (maskgen_ref.z64_rows(ks2) == rows64[10:]).all()


def test_first_diff_report():
    want = np.zeros((3 * 128, 6), np.uint32)
    got = want.copy()
    got[128 + 8 * 14 + 3, 4] = 1 << (31 - 8 * 2 - 5)
    msg = maskgen_ref.first_diff_gf2(got, want, 250)
    assert "block 1 (counter 251" in msg and "keystream byte 14, bit 4" in msg and "quad word 4" in msg and "repetition 18, player 5" in msg
    want64 = np.zeros((6, 8 * 24), np.uint64)
    got64 = want64.copy()
    got64[3, 8 * 18 + 5] = np.uint64(1) << np.uint64(40)
    msg = maskgen_ref.first_diff_z64(got64, want64, 250)
    assert "block 1 (counter 251" in msg and "bytes 8..15" in msg and "bit 40" in msg and "repetition 18, player 5" in msg
