"""Named digest sets for the Fiat-Shamir kernel's tests -- TEST INFRASTRUCTURE (numpy only).

k_fs_challenge takes the 256 transcript digests, not an opening map, so a map with a wanted edge has to be FOUND: the sets below are
np.random.default_rng(seed).integers(0, 256, (256, 32), uint8) for seeds found once, offline, by `python tests/fs_cases.py` (the
search at the bottom: seeds 0, 1, 2, ... in order, the first hit of every name; comm from the official BLAKE3 that
b3_ref.load_official() loads, the map from fs_ref).  No search runs at test time; tests/test_fs_ref_host.py checks, with the
reference alone, that every committed seed still has the property its name claims.

  empty32@P     the 32-repetition shard at position P (repetitions 32 P .. 32 P + 31) opens nothing
  empty64       a 64-repetition shard opens nothing (found inside the budget of 100 000 tries)
  crowded32     a 32-repetition shard with at least 13 opened
  crowded64     a 64-repetition shard with at least 20 opened
  ends          repetitions 0 and 255 both opened
  seamN         repetitions N and N + 1 both opened (N + 1 starts a 64-lane group of the kernel's loops)
  redraw        before the 40th distinct repetition, a repetition is drawn twice with different players
  late          after the 40th distinct repetition, inside the first 128 draws, an already opened repetition is drawn again with a
                different player: this draw must be ignored
  zeros, ones   all-zero and all-0xFF digests;  plain: nothing special

The second draw round needs fewer than 40 distinct values among 128 draws. No input is known, and none is to be hunted for."""
from __future__ import annotations

import functools

import numpy as np

import fs_ref

SEEDS = {
    "plain": 2,
    "empty32@0": 800,
    "empty32@3": 212,
    "empty32@7": 7,
    "empty64": 50626,
    "crowded32": 1322,
    "crowded64": 1436,
    "ends": 35,
    "seam63": 9,
    "seam127": 64,
    "seam191": 48,
    "redraw": 1,
    "late": 0,
}
FIXED = {"zeros": 0x00, "ones": 0xFF}
NAMES = list(SEEDS) + list(FIXED)


def random_digests(seed: int) -> np.ndarray:
    return np.random.default_rng(seed).integers(0, 256, (256, 32), dtype=np.uint8)


@functools.lru_cache(maxsize=None)
def digests(name: str) -> np.ndarray:
    d = np.full((256, 32), FIXED[name], np.uint8) if name in FIXED else random_digests(SEEDS[name])
    d.setflags(write=False)
    return d


@functools.lru_cache(maxsize=None)
def case(name: str):
    """-> (digests, comm, omit[256], done_at, draws): the reference's answers, computed once"""
    d = digests(name)
    c = fs_ref.comm(d)
    omit, done_at, drawn = fs_ref.opening(c)
    for a in (c, omit, drawn):
        a.setflags(write=False)
    return d, c, omit, done_at, drawn


def shard_counts(omit, width: int) -> np.ndarray:
    return (np.asarray(omit).reshape(-1, width) < 8).sum(axis=1)


def own_shard(name: str, omit):
    """(rep_begin, R) of the shard an empty* / crowded* set is named after; None for the other sets"""
    if name.startswith("empty32@"):
        return 32 * int(name[-1]), 32
    if name == "empty64":
        return 64 * int(np.argmin(shard_counts(omit, 64))), 64
    if name == "crowded32":
        return 32 * int(np.argmax(shard_counts(omit, 32))), 32
    if name == "crowded64":
        return 64 * int(np.argmax(shard_counts(omit, 64))), 64
    return None


def _redraw(omit, done_at, drawn) -> bool:
    first = {}
    for rep, player in drawn[:done_at + 1]:
        if rep in first and first[rep] != player:
            return True
        first.setdefault(int(rep), int(player))
    return False


def _late(omit, done_at, drawn) -> bool:
    return done_at < 127 and any(omit[rep] < 8 and omit[rep] != player for rep, player in drawn[done_at + 1:128])


def holds(name: str, omit, done_at, drawn) -> bool:
    """does the opening have the property the name claims?"""
    omit = np.asarray(omit)
    if name.startswith("empty32@"):
        return shard_counts(omit, 32)[int(name[-1])] == 0
    if name == "empty64":
        return shard_counts(omit, 64).min() == 0
    if name == "crowded32":
        return shard_counts(omit, 32).max() >= 13
    if name == "crowded64":
        return shard_counts(omit, 64).max() >= 20
    if name == "ends":
        return omit[0] < 8 and omit[255] < 8
    if name.startswith("seam"):
        n = int(name[4:])
        return omit[n] < 8 and omit[n + 1] < 8
    if name == "redraw":
        return _redraw(omit, done_at, drawn)
    if name == "late":
        return _late(omit, done_at, drawn)
    return True  # plain, zeros, ones


if __name__ == "__main__":  # the offline search that produced SEEDS
    import b3_ref

    blake3 = b3_ref.load_official()
    todo = [n for n in SEEDS if n != "plain"]
    found = {}
    def fast_opening(c):  # (the official hasher's extended output in place of fs_ref.draws: the search's fast route)
        x = np.frombuffer(blake3(fs_ref.CTX_CHALLENGE + b"\0" + c.tobytes(), n=64 * 64), np.uint8).reshape(128, 2, 16)[:, :, 0].astype(np.int64)
        x[:, 1] &= 7
        omit, seen = np.full(256, 8, np.uint8), 0
        for i, (rep, player) in enumerate(x):
            seen += omit[rep] == 8
            omit[rep] = player
            if seen == 40:
                return omit, i, x
        raise AssertionError("fewer than 40 distinct repetitions among 128 draws")

    for seed in range(100_000):
        c = np.frombuffer(blake3(random_digests(seed).tobytes()), np.uint8)
        omit, done_at, drawn = fast_opening(c)
        for n in list(todo):
            if holds(n, omit, done_at, drawn):
                found[n] = seed
                todo.remove(n)
                print(f'    "{n}": {seed},', flush=True)
        if not todo:
            break
    print("not found:", todo)
