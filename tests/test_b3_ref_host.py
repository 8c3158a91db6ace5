"""tests/b3_ref.py (the reference of tests/test_gpu_b3_kernels.py) against three implementations it shares no code with: the official
BLAKE3 C build that ROCm's libclang-cpp.so exports as llvm_blake3_hasher_* (loaded the way tests/golden/gen_golden.py loads it), the
CPU oracle's rvo_blake3_hash, and the committed known answers of tests/golden/primitives.json.  (No GPU.)"""
import ctypes as C
import json
import os

import numpy as np
import pytest

import b3_ref
from conftest import GOLDEN

LENGTHS = [0, 1, 63, 64, 65, 1023, 1024, 1025, 2047, 2048, 2049, 4072, 5 * 1024 + 1, 70001]


@pytest.fixture(scope="module")
def official():
    return b3_ref.load_official()


def streams(n, R=3, seed=0):
    """R byte strings of n bytes: the known answers' i % 251 pattern first, random bytes after it"""
    d = np.random.default_rng(1000 + 7 * n + seed).integers(0, 256, (R, n), dtype=np.uint8)
    d[0] = np.arange(n) % 251
    return d


@pytest.mark.parametrize("n", LENGTHS)
def test_hash_vs_official_and_oracle(official, oracle, n):
    data = streams(n)
    got = b3_ref.hash_bytes(data)
    buf = C.create_string_buffer(32)
    for r in range(len(data)):
        assert got[r].tobytes() == official(data[r].tobytes()), (n, r)
        oracle.lib().rvo_blake3_hash(data[r].tobytes(), C.c_size_t(n), buf)
        assert got[r].tobytes() == buf.raw, (n, r)


def test_hash_vs_known_answers():
    kats = json.load(open(os.path.join(GOLDEN, "primitives.json")))["blake3"]
    assert {0, 1, 63, 64, 65, 1023, 1024, 1025, 2048, 2049} <= {k["len"] for k in kats}
    for k in kats:
        n = k["len"]
        data = (np.arange(n) % 251).astype(np.uint8)[None, :]
        assert b3_ref.hash_bytes(data)[0].tobytes().hex() == k["hash"], n


@pytest.mark.parametrize("base", [1, 2, 3, 5, 8, 13])
@pytest.mark.parametrize("n", [1, 1024, 1025, 4072])
def test_chunk_base_vs_official(official, base, n):
    """a piece of a longer stream: `base` whole chunks in front, then n bytes hashed with chunk counters base, base + 1, ... -- the
    tree over both pieces' chaining values is the official digest of the whole message"""
    whole = streams(base * 1024 + n, seed=base)
    front = b3_ref.chunk_cvs(whole[:, :base * 1024], root_ok=False)
    back = b3_ref.chunk_cvs(whole[:, base * 1024:], base=base, root_ok=False)
    assert len(front) == base and len(back) == (n + 1023) // 1024
    got = b3_ref.digest_bytes(b3_ref.tree(np.concatenate([front, back])))
    for r in range(len(whole)):
        assert got[r].tobytes() == official(whole[r].tobytes()), (base, n, r)


def test_lone_chunk_root_flag(official):
    data = streams(100)
    with_root, without = b3_ref.chunk_cvs(data), b3_ref.chunk_cvs(data, root_ok=False)
    assert with_root.shape == without.shape == (1, 3, 8) and not (with_root == without).all(axis=-1).any()
    assert b3_ref.digest_bytes(with_root[0])[1].tobytes() == official(data[1].tobytes())
    # a non-root lone chunk is an ordinary leaf: beside a second chunk it gives the two-chunk message's digest
    two = streams(1024 + 100, seed=1)
    cvs = np.concatenate([b3_ref.chunk_cvs(two[:, :1024], root_ok=False), b3_ref.chunk_cvs(two[:, 1024:], base=1, root_ok=False)])
    assert b3_ref.digest_bytes(b3_ref.tree(cvs))[2].tobytes() == official(two[2].tobytes())


@pytest.mark.parametrize("t", [0, 1, 2**32 - 1, 2**32, 2**40 + 5, 2**64 - 1])
def test_compress_counter_words_vs_official(official, t):
    """both words of the 64-bit counter: the official hasher's output block t of a one-block message is the root compression with
    counter t (its first 32 bytes are the chaining-value half that compress() returns)"""
    for n in (0, 5, 64):
        data = streams(n, seed=3)
        pad = np.zeros((len(data), 64), np.uint8)
        pad[:, :n] = data
        flags = b3_ref.CHUNK_START | b3_ref.CHUNK_END | b3_ref.ROOT
        got = b3_ref.digest_bytes(b3_ref.compress(b3_ref.IV, pad.view("<u4"), t, n, flags))
        if t < 2**58:  # (the seek is a byte offset)
            for r in range(len(data)):
                assert got[r].tobytes() == official(data[r].tobytes(), 32, 64 * t), (t, n, r)
        # and a counter word that is not looked at would collide with the counter that has it cleared
        other = b3_ref.digest_bytes(b3_ref.compress(b3_ref.IV, pad.view("<u4"), t ^ (1 << 32), n, flags))
        assert not (got == other).all(axis=-1).any()


def test_tree_shapes():
    """the tree is the specification's, not "pair neighbours, promote the odd one": at n = 3, 5, 6, 7 the explicit nesting"""
    rng = np.random.default_rng(5)
    cv = rng.integers(0, 2**32, (7, 2, 8), dtype=np.uint32)
    P = b3_ref.parent
    assert (b3_ref.tree(cv[:1]) == cv[0]).all()
    assert (b3_ref.tree(cv[:2]) == P(cv[0], cv[1], True)).all()
    assert (b3_ref.tree(cv[:3]) == P(P(cv[0], cv[1], False), cv[2], True)).all()
    four = P(P(cv[0], cv[1], False), P(cv[2], cv[3], False), False)
    assert (b3_ref.tree(cv[:5]) == P(four, cv[4], True)).all()
    assert (b3_ref.tree(cv[:6]) == P(four, P(cv[4], cv[5], False), True)).all()
    assert (b3_ref.tree(cv[:7]) == P(four, P(P(cv[4], cv[5], False), cv[6], False), True)).all()
    assert (b3_ref.incremental(cv, [1, 0, 2, 3]) == b3_ref.tree(cv)).all()


def test_join_vs_official(official):
    rng = np.random.default_rng(6)
    d = rng.integers(0, 2**32, (4, 5, 8), dtype=np.uint32)
    got = b3_ref.join(*d)
    by = b3_ref.digest_bytes(d)
    for r in range(5):
        h2 = official(by[0, r].tobytes() + by[1, r].tobytes())
        h64 = official(by[2, r].tobytes() + by[3, r].tobytes())
        assert got[r].tobytes() == official(h2 + h64)


def test_layouts():
    rng = np.random.default_rng(7)
    R, n = 16, 5
    data = rng.integers(0, 256, (R, n), dtype=np.uint8)
    rows = b3_ref.byte_rows(data)
    assert rows.shape == (n, R // 4) and rows.dtype == np.uint32
    for r in range(R):
        for e in range(n):
            assert (int(rows[e, r // 4]) >> (24 - 8 * (r % 4))) & 0xFF == data[r, e]
    bits = rng.integers(0, 2, (R, n), dtype=np.uint8)
    brow, hashed = b3_ref.bit_rows(bits)
    assert brow.shape == (n, R // 8) and brow.dtype == np.uint8 and (hashed == bits * 255).all()
    for r in range(R):
        q, i4 = r // 4, r % 4
        for e in range(n):
            assert (int(brow[e, q >> 1]) >> (4 * (q & 1) + 3 - i4)) & 1 == bits[r, e]
    words = rng.integers(0, 256, (R, 24), dtype=np.uint8)
    cs = b3_ref.contig_streams(words, 5)
    assert cs.shape == (R, 5) and cs.dtype == np.uint64
    assert int(cs[3, 1]) == int.from_bytes(words[3, 8:16].tobytes(), "little") and int(cs[3, 4]) == 0xEEEEEEEEEEEEEEEE
    cv = rng.integers(0, 2**32, (2, R, 8), dtype=np.uint32)
    sq = b3_ref.scatter_quads(cv, [0, 3])
    assert (sq[:, 0:4] == cv[:, 0:4]).all() and (sq[:, 12:16] == cv[:, 12:16]).all() and (sq[:, 4:12] == 0xA5A5A5A5).all()
