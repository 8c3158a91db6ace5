"""Plain numpy reference of Fiat-Shamir, the proof's record layout and the fixed-size pieces of its records -- TEST INFRASTRUCTURE
(numpy only, no library import).

Written from the definitions, not from the kernels: the challenge from the reference's proof/mod.rs:68-108 (combine_hashes,
random_int, challenge_to_opening) and crypto/ro.rs:8-20 (RandomOracle), the layout from the proof format in tests/proof_mutate.py's
docstring and the comment of open_layout_of (csrc/open.inc):

    proof   = comm[32] | domain gf2 | domain z64
    domain  = u64 n_online | n_online x record | u64 n_pre | n_pre x (seed[16] | H_on[32])
    record  = omit[1] | keys[8][16], the omitted player's zeroed | u64 len, rec | u64 len, corr | u64 len, in

A shard of R repetitions writes its four sections one after the other -- gf2 online records, gf2 preprocessing records, z64 online
records, z64 preprocessing records -- from base0; `framed` puts comm and the four u64 counts around them (a whole proof).

lens = (l2r, l2c, l2i, l64r, l64c, l64i): the BYTE lengths of the three GF(2) and the three Z64 vectors of an online record.
omit: 0..7 = the opened repetition's omitted player, 8 = not opened.  tests/test_fs_ref_host.py ties this module to the CPU oracle
and to a golden proof before any GPU result is compared with it."""
from __future__ import annotations

import numpy as np

import b3_ref

TOTAL_REPS, ONLINE_REPS, PLAYERS = 256, 40, 8
CTX_CHALLENGE = b"random-oracle challenge"
PRE_RECORD = 48  # seed[16] | H_on[32]
HEAD = 1 + 128   # omit | keys


def comm(digests) -> np.ndarray:
    """combine_hashes: BLAKE3 of the 256 digests one after the other -> [32] bytes"""
    d = np.ascontiguousarray(digests, np.uint8)
    assert d.shape == (TOTAL_REPS, 32)
    return b3_ref.hash_bytes(d.reshape(1, -1))[0]


def draws(comm_bytes, first_block: int = 0, n_blocks: int = 64) -> np.ndarray:
    """the random oracle's draws out of output blocks [first_block, first_block + n_blocks) -> [2 n_blocks, 2] (rep, player) in order.
    The oracle's input is ctx || 0x00 || comm, 56 bytes: one block, so every 64-byte output block is one compression of it with the
    output-block counter.  random_int takes 16 bytes as a little-endian u128 modulo the bound: modulo 256 the first byte, modulo 8
    the first byte's low three bits; a block holds two (rep, player) pairs."""
    c = np.ascontiguousarray(comm_bytes, np.uint8)
    assert c.shape == (32,)
    msg = np.zeros(64, np.uint8)
    msg[:len(CTX_CHALLENGE)] = np.frombuffer(CTX_CHALLENGE, np.uint8)
    msg[len(CTX_CHALLENGE) + 1:len(CTX_CHALLENGE) + 33] = c
    blen = len(CTX_CHALLENGE) + 33
    t = np.arange(first_block, first_block + n_blocks, dtype=np.uint64)
    out = b3_ref.compress_xof(b3_ref.IV, msg.view("<u4"), t, blen, b3_ref.CHUNK_START | b3_ref.CHUNK_END | b3_ref.ROOT)
    by = np.ascontiguousarray(out.astype("<u4")).view(np.uint8).reshape(n_blocks, 64)
    pairs = np.stack([by[:, 0], by[:, 16] & 7, by[:, 32], by[:, 48] & 7], axis=1).reshape(2 * n_blocks, 2)
    return pairs.astype(np.int64)


def opening(comm_bytes):
    """challenge_to_opening -> (omit[256], index of the draw that reached 40 distinct repetitions, the draws up to the end of its
    round of 128).  The draws are replayed in order; a repetition drawn again takes the later player; the replay stops at 40."""
    omit = np.full(TOTAL_REPS, PLAYERS, np.uint8)
    seen, block, done_at, all_draws = 0, 0, None, []
    while done_at is None:
        d = draws(comm_bytes, block, 64)
        for i, (rep, player) in enumerate(d):
            if omit[rep] == PLAYERS:
                seen += 1
            omit[rep] = player
            if seen == ONLINE_REPS:
                done_at = 2 * block + i
                break
        all_draws.append(d)
        block += 64
    return omit, done_at, np.concatenate(all_draws)


def record_sizes(lens):
    l2r, l2c, l2i, l64r, l64c, l64i = (int(x) for x in lens)
    return HEAD + 24 + l2r + l2c + l2i, HEAD + 24 + l64r + l64c + l64i


def section_starts(n_on: int, n_pre: int, lens, base0: int, framed: bool):
    """-> ([4] starts of gf2 online, gf2 preprocessing, z64 online, z64 preprocessing; the end).  framed: base0 is where comm
    stands, and a u64 count stands in front of every section"""
    sz2, sz64 = record_sizes(lens)
    at = int(base0) + (32 if framed else 0)
    starts = []
    for size in (n_on * sz2, n_pre * PRE_RECORD, n_on * sz64, n_pre * PRE_RECORD):
        if framed:
            at += 8
        starts.append(at)
        at += size
    return starts, at


def record_table(omit_local, off2, off64, lens) -> np.ndarray:
    """the [8][R] table of records that lie at off2[r] / off64[r]: rows 0, 1 the records, rows 2..4 the starts of the gf2 rec / corr /
    in vectors, rows 5..7 those of the z64 vectors -- each vector behind its u64 length, the first behind omit | keys; zeros in rows
    2..7 for an unopened repetition (it has no vectors)"""
    omit_local = np.asarray(omit_local, np.uint8)
    R = len(omit_local)
    table = np.zeros((8, R), np.uint64)
    for r in range(R):
        col = [int(off2[r]), int(off64[r]), 0, 0, 0, 0, 0, 0]
        if omit_local[r] < PLAYERS:
            for dom in (0, 1):
                at = col[dom] + HEAD
                for v in range(3):
                    at += 8
                    col[2 + 3 * dom + v] = at
                    at += int(lens[3 * dom + v])
        table[:, r] = np.array(col, np.uint64)
    return table


def layout(omit_local, lens, base0: int, framed: bool):
    """-> (table [8][R] u64 as record_table gives it, online list {"n", "rep", "dst"}, (n_on, n_pre), end).
    The j-th opened repetition's records are the j-th of the two online sections, the j-th unopened one's the j-th of the two
    preprocessing sections.  The list: the opened repetitions in order (local numbers) with the start of each one's gf2 corrections
    vector."""
    omit_local = np.asarray(omit_local, np.uint8)
    R = len(omit_local)
    sz2, sz64 = record_sizes(lens)
    on = omit_local < PLAYERS
    n_on = int(on.sum())
    n_pre = R - n_on
    starts, end = section_starts(n_on, n_pre, lens, base0, framed)
    k = np.where(on, np.cumsum(on) - 1, np.cumsum(~on) - 1)
    off2 = [starts[0] + int(k[r]) * sz2 if on[r] else starts[1] + int(k[r]) * PRE_RECORD for r in range(R)]
    off64 = [starts[2] + int(k[r]) * sz64 if on[r] else starts[3] + int(k[r]) * PRE_RECORD for r in range(R)]
    table = record_table(omit_local, off2, off64, lens)
    rep = [int(r) for r in np.nonzero(on)[0]]
    return table, {"n": n_on, "rep": rep, "dst": [int(table[3, r]) for r in rep]}, (n_on, n_pre), end


def fields(omit_local, table, lens) -> list:
    """[(name, start, length)] of every field of the shard's records, for describe()"""
    out = []
    for r, om in enumerate(np.asarray(omit_local, np.uint8)):
        for dom, dn in enumerate(("gf2", "z64")):
            at = int(table[dom, r])
            if om < PLAYERS:
                out += [(f"repetition {r}, {dn} record: omit", at, 1), (f"repetition {r}, {dn} record: keys", at + 1, 128)]
                for v, vn in enumerate(("rec", "corr", "in")):
                    s = int(table[2 + 3 * dom + v, r])
                    out += [(f"repetition {r}, {dn} record: length of {vn}", s - 8, 8), (f"repetition {r}, {dn} record: vector {vn}", s, int(lens[3 * dom + v]))]
            else:
                out += [(f"repetition {r}, {dn} preprocessing record: seed", at, 16), (f"repetition {r}, {dn} preprocessing record: H_on", at + 16, 32)]
    return out


def describe(got, want, named_fields) -> str:
    """where two buffers first differ, and the field that byte lies in"""
    idx = np.nonzero(np.asarray(got) != np.asarray(want))[0]
    if not len(idx):
        return "equal"
    x = int(idx[0])
    where = next((f"{n}, byte {x - s} of {ln}" for n, s, ln in named_fields if s <= x < s + ln), "outside every field")
    return f"first wrong byte at offset {x} ({where}): got 0x{int(got[x]):02x}, want 0x{int(want[x]):02x}; {len(idx)} of {len(want)} bytes differ"


def _u64le(v: int) -> bytes:
    return int(v).to_bytes(8, "little")


def _raw(b) -> bytes:
    return b if isinstance(b, bytes) else np.asarray(b, np.uint8).tobytes()


def digest_rows(words_or_bytes, R: int) -> np.ndarray:
    """[R][8] u32 words (a digest's bytes are its words little-endian) or [R][32] bytes -> [R][32] bytes"""
    a = np.asarray(words_or_bytes)
    if a.dtype == np.uint8:
        return a.reshape(R, 32)
    return np.ascontiguousarray(a.astype("<u4")).view(np.uint8).reshape(R, 32)


def heads(omit, seeds, keys, on2, on64, table, lens) -> dict:
    """{offset: bytes} of every fixed-size piece of the shard's records.  seeds [R][16], keys [R][128], on2 / on64 [R] digests of the
    online transcripts (H_on of the two domains).  Online record: omit | keys with the omitted player's 16 bytes zeroed | u64 length of
    the first vector; then the u64 length in front of the second and of the third vector.  Preprocessing record: seed | H_on."""
    omit = np.asarray(omit, np.uint8)
    R = len(omit)
    seeds = np.asarray(seeds, np.uint8).reshape(R, 16)
    keys = np.asarray(keys, np.uint8).reshape(R, 128)
    h_on = (digest_rows(on2, R), digest_rows(on64, R))
    table = np.asarray(table, np.uint64)
    out = {}
    for dom in (0, 1):
        lr, lc, li = (int(x) for x in lens[3 * dom:3 * dom + 3])
        for r in range(R):
            at = int(table[dom, r])
            if omit[r] < PLAYERS:
                k = keys[r].copy()
                k[16 * int(omit[r]):16 * int(omit[r]) + 16] = 0
                out[at] = bytes([int(omit[r])]) + k.tobytes() + _u64le(lr)
                out[int(table[2 + 3 * dom + 1, r]) - 8] = _u64le(lc)
                out[int(table[2 + 3 * dom + 2, r]) - 8] = _u64le(li)
            else:
                out[at] = seeds[r].tobytes() + h_on[dom][r].tobytes()
    return out


def frame(comm_bytes, n_on: int, n_pre: int, lens, base0: int = 0) -> dict:
    """{offset: bytes} of a framed proof's comm and its four u64 counts"""
    starts, _ = section_starts(n_on, n_pre, lens, base0, True)
    out = {int(base0): _raw(comm_bytes)}
    for k, s in enumerate(starts):
        out[s - 8] = _u64le(n_pre if k % 2 else n_on)
    return out


def mailbox(comm_bytes, omit_all, n_on: int, n_pre: int) -> np.ndarray:
    """the words the early path's host reads: comm, the whole opening map, the shard's two counts -- 8 + 64 + 2 u32 little-endian"""
    body = _raw(comm_bytes) + _raw(omit_all)
    assert len(body) == 32 + TOTAL_REPS
    return np.concatenate([np.frombuffer(body, "<u4"), np.array([n_on, n_pre], "<u4")]).astype(np.uint32)


def image(fill: int, size: int, pieces: dict):
    """a buffer of `size` fill bytes with every piece at its offset"""
    img = np.full(size, fill, np.uint8)
    for at, b in pieces.items():
        assert 0 <= at and at + len(b) <= size, (at, len(b), size)
        img[at:at + len(b)] = np.frombuffer(bytes(b), np.uint8)
    return img
