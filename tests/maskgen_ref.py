"""Plain numpy reference of the mask generators' device rows -- TEST INFRASTRUCTURE.

Built from the definition of the layout, not from the kernels: the only cipher here is the CPU oracle's AES-128-CTR
(oracle_lib.expand_seed, oracle_lib.prg_blocks).  A shard of R repetitions (R a multiple of 4) has NQ = R / 4 quad words;
repetition r sits in quad word q = r // 4 at position r % 4, its player p in slot 8 * (r % 4) + p of the word's 32.

  GF(2)  rows[128 * jl + 8 * i + b, q], bit 31 - 8 * (r % 4) - p  =  bit 7 - b of keystream byte i of block first_block + jl
         of (repetition r, player p); uint32 [n_blocks * 128, NQ]
  Z64    rows[2 * jl + h, 8 * r + p]  =  the little-endian u64 of keystream bytes 8h .. 8h + 8 of that block;
         uint64 [2 * n_blocks, 8 * R]

An omitted player's keystream counts as zero in both.  tests/test_maskgen_ref_host.py ties this module to the oracle's
share generators and the committed golden shares before any GPU result is compared with it.
"""
from __future__ import annotations

import numpy as np

import oracle_lib


def keystream(seeds, omit, first_block: int, n_blocks: int) -> np.ndarray:
    """[R, 8, n_blocks, 16] keystream bytes of (repetition, player), zero for a repetition's omitted player.
    omit: None (nobody omitted) or [R] values 0..7 / 8 = none."""
    seeds = np.asarray(seeds, np.uint8).reshape(-1, 16)
    R = len(seeds)
    keys = np.stack([oracle_lib.expand_seed(s) for s in seeds])  # [R, 8, 16]
    ks = oracle_lib.prg_blocks(keys.reshape(R * 8, 16), first_block, n_blocks).reshape(R, 8, n_blocks, 16)
    return mask_omitted(ks, omit)


def keystream_from_keys(keys, omit, first_block: int, n_blocks: int) -> np.ndarray:
    """keystream() from player keys [R, 8, 16] instead of repetition seeds"""
    keys = np.asarray(keys, np.uint8).reshape(-1, 8, 16)
    ks = oracle_lib.prg_blocks(keys.reshape(-1, 16), first_block, n_blocks).reshape(len(keys), 8, n_blocks, 16)
    return mask_omitted(ks, omit)


def mask_omitted(ks: np.ndarray, omit) -> np.ndarray:
    if omit is None:
        return ks
    omit = np.asarray(omit)
    assert omit.shape == (ks.shape[0],) and omit.max() <= 8
    ks = ks.copy()
    for r in np.nonzero(omit < 8)[0]:
        ks[r, omit[r]] = 0
    return ks


def gf2_rows(ks: np.ndarray) -> np.ndarray:
    """uint32 [n_blocks * 128, NQ] from keystream()'s bytes"""
    R, _, n, _ = ks.shape
    assert R % 4 == 0
    nq = R // 4
    bits = np.unpackbits(ks, axis=-1).reshape(nq, 4, 8, n, 16, 8)  # [q, r % 4, p, jl, i, b]: entry b of unpackbits = bit 7 - b
    bits = np.ascontiguousarray(bits.transpose(3, 4, 5, 0, 1, 2)).reshape(n * 128, nq, 32)  # last axis: slot 8 * (r % 4) + p
    # slot s is bit 31 - s: the 32 slots packed MSB-first are the word's four bytes from the most significant down
    return np.packbits(bits, axis=-1).view(">u4").reshape(n * 128, nq).astype(np.uint32)


def z64_rows(ks: np.ndarray) -> np.ndarray:
    """uint64 [2 * n_blocks, 8 * R] from keystream()'s bytes"""
    R, _, n, _ = ks.shape
    w = np.ascontiguousarray(ks).view("<u8").reshape(R, 8, n, 2)  # [r, p, jl, h]
    return np.ascontiguousarray(w.transpose(2, 3, 0, 1)).reshape(2 * n, R * 8).astype(np.uint64)


# ---- the layouts of rv_hook_sharegen_gf2 / rv_hook_sharegen_z64 (8 repetitions from block 0) ----
def sharegen_gf2_layout(rows: np.ndarray, n: int) -> np.ndarray:
    """n packed u64 shares: quad word 0 in the high half, quad word 1 in the low half"""
    assert rows.shape[1] == 2
    return (rows[:n, 0].astype(np.uint64) << np.uint64(32)) | rows[:n, 1].astype(np.uint64)


def sharegen_z64_layout(rows: np.ndarray, n: int) -> np.ndarray:
    """[n, 8 repetitions, 8 players] u64"""
    assert rows.shape[1] == 64
    return rows[:n].reshape(n, 8, 8)


# ---- where two row arrays first differ ----
def first_diff_gf2(got: np.ndarray, want: np.ndarray, first_block: int) -> str:
    idx = np.argwhere(got != want)
    if not len(idx):
        return "equal"
    row, q = (int(x) for x in idx[0])
    x = int(got[row, q]) ^ int(want[row, q])
    bit = x.bit_length() - 1
    s = 31 - bit
    return (f"block {row // 128} (counter {first_block + row // 128} = 0x{first_block + row // 128:06x}), row {row % 128} (keystream byte "
            f"{row % 128 // 8}, bit {7 - row % 8}), quad word {q}, bit {bit} (repetition {4 * q + s // 8}, player {s % 8}): "
            f"got 0x{int(got[row, q]):08x}, want 0x{int(want[row, q]):08x}; {len(idx)} of {got.size} words differ")


def first_diff_z64(got: np.ndarray, want: np.ndarray, first_block: int) -> str:
    idx = np.argwhere(got != want)
    if not len(idx):
        return "equal"
    row, slot = (int(x) for x in idx[0])
    x = int(got[row, slot]) ^ int(want[row, slot])
    return (f"block {row // 2} (counter {first_block + row // 2} = 0x{first_block + row // 2:06x}), row {row % 2} (keystream bytes "
            f"{8 * (row % 2)}..{8 * (row % 2) + 7}), quad word {slot // 32}, bit {x.bit_length() - 1} of slot {slot} (repetition {slot // 8}, "
            f"player {slot % 8}): got 0x{int(got[row, slot]):016x}, want 0x{int(want[row, slot]):016x}; {len(idx)} of {got.size} words differ")
