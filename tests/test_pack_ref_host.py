"""The opening vectors' numpy reference (tests/pack_ref.py) against the CPU oracle's Pack / PackSelected (gf2/recon.rs:189-239,
gf2/share.rs:87-149) and their inverses, before tests/test_gpu_pack.py compares any GPU result with it.  Host only.

The oracle packs one group of 8 repetitions of packed u64 words; as row words that is R = 8, NQ = 2, quad word 0 in the high half
(the mapping tests/maskgen_ref.py fixes for the shares).  Wider shards are their groups side by side, which is checked here too."""
import numpy as np
import pytest

import maskgen_ref
import pack_ref

LENGTHS = [0, 1, 7, 8, 9, 64, 1001]
MAPS = [
    [3, 0, 7, 5, 1, 2, 6, 4],   # every repetition opened, every player once
    [8, 2, 8, 8, 7, 0, 8, 5],   # some not opened
    [8, 8, 8, 8, 8, 8, 8, 0],   # the last one alone
    [8] * 8,                    # none
]


def _shares(oracle, n, seed):
    """n packed u64 shares of one group from the oracle's share generator, and the same as rows [n, 2]"""
    rng = np.random.default_rng(seed)
    keys = rng.integers(0, 256, (8, 8, 16), dtype=np.uint8)
    words = oracle.sharegen_gf2(keys, [8] * 8, n) if n else np.zeros(0, np.uint64)
    rows = pack_ref.rows_from_u64(words)
    if n:
        ks = maskgen_ref.keystream_from_keys(keys, None, 0, (n + 127) // 128)
        assert (rows == maskgen_ref.gf2_rows(ks)[:n]).all()  # the row mapping is maskgen_ref's
    return words, rows


@pytest.mark.parametrize("n", LENGTHS)
def test_share_pack_selected_equals_oracle(oracle, n):
    words, rows = _shares(oracle, n, 100 + n)
    for omit in MAPS:
        want = oracle.gf2_share_pack_selected(words, omit)
        got = pack_ref.pack_rows(rows, omit, 0)
        assert sorted(got) == [r for r in range(8) if omit[r] < 8]
        for r in range(8):
            if omit[r] < 8:
                assert len(want[r]) == n // 8 + 1 and got[r].tobytes() == want[r], (n, omit, r)
            else:
                assert want[r] == b""
        if all(o < 8 for o in omit):
            # the oracle's inverse gives the shares with nothing but the selected players' bits: so does the reference's
            back = oracle.gf2_share_unpack_selected(want, omit)
            mine = pack_ref.unpack_rows(got, omit, len(back), 2, 0)
            assert (pack_ref.u64_from_rows(mine) == back).all() and not back[n:].any()
        keep = sum(1 << (63 - (8 * r + o)) for r, o in enumerate(omit) if o < 8)
        mine = pack_ref.unpack_rows(got, omit, n + 11, 2, 0)
        assert (pack_ref.u64_from_rows(mine)[:n] == (words & np.uint64(keep))).all() and not mine[n:].any()


@pytest.mark.parametrize("n", LENGTHS)
def test_recon_pack_equals_oracle(oracle, n):
    rng = np.random.default_rng(200 + n)
    items = rng.integers(0, 2, (n, 8), dtype=np.uint8)
    rows = pack_ref.recon_rows_from_items(items)
    words = pack_ref.u64_from_rows(rows)
    if n:
        assert words[0] == sum(0xFF << (56 - 8 * r) for r in range(8) if items[0, r])  # ReconGF2: repetition r in byte 7 - r
    bits = pack_ref.bitstream_from_items(items)
    for omit in MAPS:
        sel = [int(o < 8) for o in omit]
        want = oracle.gf2_recon_pack(words, sel)
        got = pack_ref.pack_rows(rows, omit, 1)
        from_bits = pack_ref.pack_bitstream(bits, pack_ref.opened(omit))
        for r in range(8):
            if sel[r]:
                assert len(want[r]) == n // 8 + 1
                assert got[r].tobytes() == want[r] and from_bits[r].tobytes() == want[r], (n, omit, r)
            else:
                assert want[r] == b"" and r not in got and r not in from_bits
        mine = pack_ref.unpack_rows(got, omit, n + 11, 2, 1)
        mask = pack_ref.recon_rows_from_items(np.tile(np.array(sel, np.uint8), (n, 1)))
        assert (mine[:n] == (rows & mask)).all() and not mine[n:].any()
    full = oracle.gf2_recon_pack(words, [1] * 8)
    back = oracle.gf2_recon_unpack(full)
    mine = pack_ref.unpack_rows({r: np.frombuffer(full[r], np.uint8) for r in range(8)}, [0] * 8, len(back), 2, 1)
    assert len(back) == 8 * (n // 8 + 1) and (pack_ref.u64_from_rows(mine) == back).all() and (back[:n] == words).all()


def test_row_index_list_and_wide_shards():
    """a row-index list packs the listed rows in list order, and a wide shard is its groups of 8 side by side"""
    rng = np.random.default_rng(3)
    R, n_rows, n = 24, 50, 37
    stream = rng.integers(0, 2**32, (n_rows, R // 4), dtype=np.uint64).astype(np.uint32)
    ids = rng.integers(0, n_rows, n)
    omit = rng.integers(0, 9, R)
    for kind in (0, 1):
        got = pack_ref.pack_rows(stream, omit, kind, ids)
        for g in range(R // 8):
            part = pack_ref.pack_rows(stream[ids][:, 2 * g:2 * g + 2], omit[8 * g:8 * g + 8], kind)
            assert {8 * g + r: v.tobytes() for r, v in part.items()} == {r: v.tobytes() for r, v in got.items() if r // 8 == g}
    items = rng.integers(0, 2, (n, R), dtype=np.uint8)
    bits = pack_ref.bitstream_from_items(items)
    assert bits.shape == (n, R // 8)
    for r in range(R):
        assert (pack_ref.bitstream_items(bits, r) == items[:, r]).all()
    assert bits[0, 1] == sum(int(items[0, 8 + 3 - k]) << k for k in range(4)) | sum(int(items[0, 12 + 3 - k]) << (4 + k) for k in range(4))


def test_first_item_and_short_vectors():
    rng = np.random.default_rng(4)
    vec = rng.integers(0, 256, 9, dtype=np.uint8)
    allbits = np.unpackbits(vec)
    for first in (0, 1, 7, 8, 13, 71, 72, 100):
        got = pack_ref.unpack_items(vec, first, 20)
        want = np.concatenate([allbits[first:first + 20], np.zeros(20, np.uint8)])[:20]
        assert (got == want).all()
    assert not pack_ref.unpack_items(vec[:0], 0, 5).any()
    assert pack_ref.pack_items([]).tobytes() == b"\0" and pack_ref.pack_items([1] * 8).tobytes() == b"\xff\0"
    assert pack_ref.pack_items([1, 0, 0, 0, 0, 0, 0, 0, 1]).tobytes() == b"\x80\x80"


def test_z64_vectors():
    vals = np.array([0, 2**64 - 1, 1 << 63, 0x0102030405060708], np.uint64)
    vec = pack_ref.pack64(vals)
    assert vec.tobytes()[24:] == bytes([8, 7, 6, 5, 4, 3, 2, 1]) and len(vec) == 32
    assert (pack_ref.unpack64(vec, 4) == vals).all()
    assert (pack_ref.unpack64(vec, 6) == np.concatenate([vals, np.zeros(2, np.uint64)])).all()
    assert (pack_ref.unpack64(vec[:31], 4) == np.array([0, 2**64 - 1, 1 << 63, 0], np.uint64)).all()  # a partial item reads as zero
    assert (pack_ref.unpack64(vec[:7], 2) == 0).all() and len(pack_ref.pack64([])) == 0


def test_first_diff_reports():
    vecs = {5: np.arange(10, dtype=np.uint8), 9: np.arange(4, dtype=np.uint8)}
    want, spans = pack_ref.image(0xA5, 64, vecs, {5: 3, 9: 40})
    assert (want[:3] == 0xA5).all() and want[3 + 9] == 9 and want[13] == 0xA5
    got = want.copy()
    assert pack_ref.first_diff_bytes(got, want, spans) == "equal"
    got[3 + 7] ^= 0x10
    msg = pack_ref.first_diff_bytes(got, want, spans)
    assert "repetition 5, byte 7 of 10 (items 56..63)" in msg and "got 0x17, want 0x07" in msg
    got = want.copy()
    got[44] = 0
    msg = pack_ref.first_diff_bytes(got, want, spans)
    assert "outside every vector" in msg and "offset 44" in msg and "repetition 9" in msg
    rows = np.zeros((20, 6), np.uint32)
    bad = rows.copy()
    bad[13, 4] = 1 << (31 - 8 * 2 - 5)
    msg = pack_ref.first_diff_rows(bad, rows)
    assert "item 13 (byte 1, bit 2" in msg and "quad word 4, repetition 18" in msg
    r64 = np.zeros((3, 8), np.uint64)
    bad = r64.copy()
    bad[2, 7] = 5
    assert "item 2, repetition 7" in pack_ref.first_diff_rows(bad, r64, per_quad=1)
