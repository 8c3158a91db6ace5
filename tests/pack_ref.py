"""Plain numpy reference of the opening vectors and their inverse -- TEST INFRASTRUCTURE.

Written from the definition (the reference's algebra/mod.rs Pack / PackSelected and their implementations gf2/share.rs:87-149,
gf2/recon.rs:189-239, z64/share.rs:36-88, z64/recon.rs:45-104), not from the kernels.  A shard of R repetitions has rows of
NQ = R / 4 quad words (uint32); repetition r = 4q + i sits in quad word q, its player p at bit 31 - 8i - p (tests/maskgen_ref.py).

  vector       n items -> n // 8 + 1 bytes, item j at bit 7 - j % 8 of byte j // 8, the rest zero (the reference always emits the
               chunk of the remainder, so n % 8 == 0 ends in a whole zero byte)
  kind 0       PackSelected of shares: the item is bit 31 - 8i - omit[r] of the row's quad word (the omitted player's share)
  kind 1       Pack of reconstructions: the item is the low bit of the repetition's 0x00 / 0xFF byte, bit 24 - 8i
  bit stream   the device's bit-per-repetition form of reconstructions, [n][NQ / 2] bytes: quad q is nibble q % 2 of byte q // 2
               (even quad = low nibble), repetition 4q + 3 - k at nibble bit k
  Z64          8 bytes little-endian per item, 8 n bytes
  unpack       items past a vector's end are zero; a Z64 item that is not whole is zero; rows hold nothing but the opened
               repetitions' bits (kind 0: at the omitted player's bit; kind 1: smeared over the byte)

omit[R]: 0..7 = the opened repetition's omitted player, 8 = not opened.  tests/test_pack_ref_host.py ties this module to the CPU
oracle's Pack / PackSelected before any GPU result is compared with it.
"""
from __future__ import annotations

import numpy as np


def n_bytes(n_items: int) -> int:
    return n_items // 8 + 1


def opened(omit) -> list[int]:
    return [int(r) for r in np.nonzero(np.asarray(omit) < 8)[0]]


def pack_items(bits) -> np.ndarray:
    """n items (0 / 1) -> the n // 8 + 1 bytes of their vector"""
    bits = np.asarray(bits, np.uint8)
    padded = np.zeros(8 * n_bytes(len(bits)), np.uint8)
    padded[:len(bits)] = bits
    return np.packbits(padded)


def unpack_items(vec, first_item: int, n_items: int) -> np.ndarray:
    """items [first_item, first_item + n_items) of a vector's bytes, zero past its end"""
    bits = np.unpackbits(np.asarray(vec, np.uint8))
    out = np.zeros(n_items, np.uint8)
    have = bits[first_item:first_item + n_items]
    out[:len(have)] = have
    return out


def row_items(rows, r: int, kind: int, omit_r: int) -> np.ndarray:
    """repetition r's item of every row of rows [n, NQ] uint32"""
    q, i = divmod(r, 4)
    sh = 31 - 8 * i - omit_r if kind == 0 else 24 - 8 * i
    return ((np.asarray(rows, np.uint32)[:, q] >> np.uint32(sh)) & np.uint32(1)).astype(np.uint8)


def pack_rows(stream, omit, kind: int, row_ids=None) -> dict:
    """{r: vector bytes} of the opened repetitions, over rows row_ids of the stream (None: all of them, in order)"""
    out = {}
    for r in opened(omit):
        items = row_items(stream, r, kind, int(omit[r]))
        out[r] = pack_items(items if row_ids is None else items[np.asarray(row_ids, np.int64)])
    return out


def bitstream_items(bits, r: int) -> np.ndarray:
    """repetition r's item of every row of a bit stream [n, NQ / 2] uint8"""
    q, i = divmod(r, 4)
    k = 3 - i
    return ((np.asarray(bits, np.uint8)[:, q // 2] >> np.uint8(4 * (q % 2) + k)) & np.uint8(1)).astype(np.uint8)


def pack_bitstream(bits, reps) -> dict:
    """{r: vector bytes} of the repetitions `reps` of a bit stream"""
    return {int(r): pack_items(bitstream_items(bits, int(r))) for r in reps}


def bitstream_from_items(items) -> np.ndarray:
    """items [n, R] (0 / 1) -> the bit stream [n, R / 8]"""
    items = np.asarray(items, np.uint8)
    n, R = items.shape
    out = np.zeros((n, R // 8), np.uint8)
    for r in range(R):
        q, i = divmod(r, 4)
        out[:, q // 2] |= items[:, r] << np.uint8(4 * (q % 2) + 3 - i)
    return out


def recon_rows_from_items(items) -> np.ndarray:
    """items [n, R] (0 / 1) -> reconstruction rows [n, R / 4] uint32, a 0x00 / 0xFF byte per repetition"""
    items = np.asarray(items, np.uint32)
    n, R = items.shape
    out = np.zeros((n, R // 4), np.uint32)
    for r in range(R):
        q, i = divmod(r, 4)
        out[:, q] |= (items[:, r] * np.uint32(0xFF)) << np.uint32(24 - 8 * i)
    return out


def unpack_rows(vecs: dict, omit, n_items: int, nq: int, kind: int, first_item: int = 0) -> np.ndarray:
    """rows [n_items, nq] uint32 rebuilt from {r: vector bytes}; row 0 is item first_item of the vectors"""
    out = np.zeros((n_items, nq), np.uint32)
    for r in opened(omit):
        q, i = divmod(r, 4)
        val = np.uint32(1 << (31 - 8 * i - int(omit[r]))) if kind == 0 else np.uint32(0xFF << (24 - 8 * i))
        out[:, q] |= unpack_items(vecs[r], first_item, n_items).astype(np.uint32) * val
    return out


def pack64(values) -> np.ndarray:
    return np.ascontiguousarray(np.asarray(values, np.uint64).astype("<u8")).view(np.uint8).copy()


def unpack64(vec, n_items: int) -> np.ndarray:
    vec = np.asarray(vec, np.uint8)
    whole = min(len(vec) // 8, n_items)
    out = np.zeros(n_items, np.uint64)
    out[:whole] = np.ascontiguousarray(vec[:8 * whole]).view("<u8")
    return out


# ---- the packed u64 forms of the oracle (one group of 8 repetitions: quad word 0 in the high half) ----
def rows_from_u64(words) -> np.ndarray:
    words = np.asarray(words, np.uint64)
    return np.stack([(words >> np.uint64(32)).astype(np.uint32), (words & np.uint64(0xFFFFFFFF)).astype(np.uint32)], axis=1)


def u64_from_rows(rows) -> np.ndarray:
    rows = np.asarray(rows, np.uint32)
    assert rows.shape[1] == 2
    return (rows[:, 0].astype(np.uint64) << np.uint64(32)) | rows[:, 1].astype(np.uint64)


# ---- expected images and where two of them first differ ----
def image(fill: int, size: int, vecs: dict, at) -> tuple:
    """a buffer of `size` fill bytes with vector r at at[r]; also the spans [(r, start, length)] for first_diff_bytes"""
    img = np.full(size, fill, np.uint8)
    spans = []
    for r, v in vecs.items():
        a = int(at[r])
        assert a + len(v) <= size
        img[a:a + len(v)] = v
        spans.append((r, a, len(v)))
    return img, spans


def first_diff_bytes(got, want, spans) -> str:
    idx = np.nonzero(np.asarray(got) != np.asarray(want))[0]
    if not len(idx):
        return "equal"
    x = int(idx[0])
    tail = f"got 0x{int(got[x]):02x}, want 0x{int(want[x]):02x}; {len(idx)} of {len(want)} bytes differ"
    for r, a, n in spans:
        if a <= x < a + n:
            b = x - a
            return f"repetition {r}, byte {b} of {n} (items {8 * b}..{8 * b + 7}), buffer offset {x}: {tail}"
    near = min(spans, key=lambda s: min(abs(x - s[1]), abs(x - (s[1] + s[2] - 1)))) if spans else None
    where = "" if near is None else f" (nearest vector: repetition {near[0]} at [{near[1]}, {near[1] + near[2]}))"
    return f"byte outside every vector, buffer offset {x}{where}: {tail}"


def first_diff_rows(got, want, per_quad: int = 4) -> str:
    """rows [n, width]: per_quad = 4 repetitions per uint32 quad word, or 1 for Z64 rows [n, R] uint64"""
    idx = np.argwhere(np.asarray(got) != np.asarray(want))
    if not len(idx):
        return "equal"
    it, q = (int(v) for v in idx[0])
    g, w = int(got[it, q]), int(want[it, q])
    if per_quad == 4:
        i = (31 - ((g ^ w).bit_length() - 1)) // 8
        return (f"item {it} (byte {it // 8}, bit {7 - it % 8} of the vectors), quad word {q}, repetition {4 * q + i}: got 0x{g:08x}, "
                f"want 0x{w:08x}; {len(idx)} of {np.asarray(want).size} words differ")
    return f"item {it}, repetition {q}: got 0x{g:016x}, want 0x{w:016x}; {len(idx)} of {np.asarray(want).size} words differ"
