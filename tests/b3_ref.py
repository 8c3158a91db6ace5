"""BLAKE3 at the level the transcript kernels work at (b3_tree.hip, z64.hip: k_b3_chunks_contig), in numpy, vectorised over
repetitions: the compression function, chunk chaining values, parents, the tree AS THE SPECIFICATION STATES IT, the digest join, and
the three layouts the kernels read.  Written from the BLAKE3 paper (section 2: compression function, chunk chaining values, the tree
"left subtree = the largest power of two of chunks strictly below the total"); it shares no code with the kernels, with
oracle/rv_blake3.c or with the official C implementation.  tests/test_b3_ref_host.py ties it to all three.

Chaining values and digests are uint32 words ([..., 8]); a digest's bytes are its words little-endian."""
import ctypes as C
import os

import numpy as np

IV = np.array([0x6A09E667, 0xBB67AE85, 0x3C6EF372, 0xA54FF53A, 0x510E527F, 0x9B05688C, 0x1F83D9AB, 0x5BE0CD19], np.uint32)
MSG_PERMUTATION = (2, 6, 3, 10, 7, 0, 4, 13, 1, 11, 12, 5, 9, 14, 15, 8)
CHUNK_START, CHUNK_END, PARENT, ROOT = 1, 2, 4, 8
CHUNK_LEN, BLOCK_LEN = 1024, 64


def _rotr(x, n):
    return (x >> np.uint32(n)) | (x << np.uint32(32 - n))


def _g(v, a, b, c, d, mx, my):
    v[a] = v[a] + v[b] + mx
    v[d] = _rotr(v[d] ^ v[a], 16)
    v[c] = v[c] + v[d]
    v[b] = _rotr(v[b] ^ v[c], 12)
    v[a] = v[a] + v[b] + my
    v[d] = _rotr(v[d] ^ v[a], 8)
    v[c] = v[c] + v[d]
    v[b] = _rotr(v[b] ^ v[c], 7)


def _state(cv, m, t, blen, flags):
    """the sixteen state words after the seven rounds, before the feed-forward"""
    cv = np.asarray(cv, np.uint32)
    m = np.asarray(m, np.uint32)
    lead = np.broadcast_shapes(cv.shape[:-1], m.shape[:-1], np.shape(t), np.shape(blen), np.shape(flags))
    t = np.broadcast_to(np.asarray(t, np.uint64), lead)
    bc = lambda x: np.broadcast_to(np.asarray(x, np.uint32), lead).copy()  # noqa: E731
    v = [bc(cv[..., i]) for i in range(8)] + [bc(IV[i]) for i in range(4)]
    v += [(t & np.uint64(0xFFFFFFFF)).astype(np.uint32), (t >> np.uint64(32)).astype(np.uint32), bc(blen), bc(flags)]
    w = [bc(m[..., i]) for i in range(16)]
    with np.errstate(over="ignore"):
        for rnd in range(7):
            _g(v, 0, 4, 8, 12, w[0], w[1])
            _g(v, 1, 5, 9, 13, w[2], w[3])
            _g(v, 2, 6, 10, 14, w[4], w[5])
            _g(v, 3, 7, 11, 15, w[6], w[7])
            _g(v, 0, 5, 10, 15, w[8], w[9])
            _g(v, 1, 6, 11, 12, w[10], w[11])
            _g(v, 2, 7, 8, 13, w[12], w[13])
            _g(v, 3, 4, 9, 14, w[14], w[15])
            if rnd < 6:
                w = [w[p] for p in MSG_PERMUTATION]
    return v


def compress(cv, m, t, blen, flags):
    """cv [..., 8], m [..., 16] uint32 words; t (64-bit counter), blen, flags: scalars or arrays that broadcast against the
    leading dimensions -> the new chaining value [..., 8] (the first half of the output block)"""
    v = _state(cv, m, t, blen, flags)
    return np.stack([v[i] ^ v[i + 8] for i in range(8)], axis=-1)


def compress_xof(cv, m, t, blen, flags):
    """the whole 64-byte output block [..., 16] (extended output: t is the output-block counter): the chaining value's half, then the
    state's upper half with the input chaining value fed forward"""
    v = _state(cv, m, t, blen, flags)
    cv = np.asarray(cv, np.uint32)
    return np.stack([v[i] ^ v[i + 8] for i in range(8)] + [v[i + 8] ^ cv[..., i] for i in range(8)], axis=-1)


def n_chunks(n_bytes):
    return 1 if n_bytes == 0 else (n_bytes + CHUNK_LEN - 1) // CHUNK_LEN


def chunk_cvs(data, base=0, root_ok=True):
    """data [R, n] bytes, one stream per repetition -> [n_chunks, R, 8].  The stream is a piece of a longer one whose first chunk has
    counter `base`; an empty stream is one empty chunk; a lone chunk carries ROOT only with root_ok."""
    data = np.ascontiguousarray(data, np.uint8)
    R, n = data.shape
    nc = n_chunks(n)
    pad = np.zeros((R, nc * CHUNK_LEN), np.uint8)
    pad[:, :n] = data
    words = pad.view("<u4").reshape(R, nc, 16, 16).transpose(1, 0, 2, 3)  # [chunk][rep][block][word]
    lens = np.minimum(CHUNK_LEN, n - CHUNK_LEN * np.arange(nc)).clip(min=0)  # bytes of every chunk
    nblk = np.maximum(1, (lens + BLOCK_LEN - 1) // BLOCK_LEN)
    t = (np.arange(nc, dtype=np.uint64) + np.uint64(base))[:, None]
    cv = np.broadcast_to(IV, (nc, R, 8)).copy()
    for b in range(16):
        live = b < nblk
        if not live.any():
            break
        blen = np.clip(lens - BLOCK_LEN * b, 0, BLOCK_LEN)
        last = b + 1 == nblk
        flags = (CHUNK_START if b == 0 else 0) | np.where(last, CHUNK_END, 0) | np.where(last & (nc == 1) & bool(root_ok), ROOT, 0)
        new = compress(cv, words[:, :, b, :], t, blen[:, None], flags[:, None])
        cv = np.where(live[:, None, None], new, cv)
    return cv


def parent(l, r, root):
    return compress(IV, np.concatenate([np.asarray(l, np.uint32), np.asarray(r, np.uint32)], axis=-1), 0, BLOCK_LEN, PARENT | (ROOT if root else 0))


def _subtree(cvs, root):
    n = len(cvs)
    if n == 1:
        return cvs[0]
    if n & (n - 1) == 0:  # a complete subtree: level by level IS the definition
        while len(cvs) > 2:
            cvs = parent(cvs[0::2], cvs[1::2], False)
        return parent(cvs[0], cvs[1], root)
    left = 1 << ((n - 1).bit_length() - 1)  # the largest power of two strictly below n
    return parent(_subtree(cvs[:left], False), _subtree(cvs[left:], False), root)


def tree(cvs):
    """cvs [n, R, 8] chunk chaining values -> the root [R, 8]; ROOT goes on the last merge only (a lone chunk is its own root: its
    chaining value was computed with ROOT already)"""
    cvs = np.asarray(cvs, np.uint32)
    assert cvs.ndim == 3 and len(cvs) >= 1
    return _subtree(cvs, True)


def incremental(cvs, cuts):
    """the streaming hasher's answer however the chaining values arrive: the tree over all of them (the binary counter is the
    kernels' business, not the reference's)"""
    assert sum(cuts) == len(cvs) - 1
    return tree(cvs)


def digest_bytes(words):
    """[..., 8] words -> [..., 32] bytes"""
    return np.ascontiguousarray(np.asarray(words, np.uint32).astype("<u4")).view(np.uint8).reshape(*np.shape(words)[:-1], 32)


def hash_bytes(data):
    """BLAKE3 of every row of data [R, n] -> [R, 32] bytes"""
    return digest_bytes(tree(chunk_cvs(data)))


def join(pre2, on2, pre64, on64):
    """h = B3(B3(pre2 || on2) || B3(pre64 || on64)) per repetition: four [R, 8] digests -> [R, 32] bytes"""
    cat = lambda a, b: np.concatenate([digest_bytes(a), digest_bytes(b)], axis=1)  # noqa: E731
    h2 = chunk_cvs(cat(pre2, on2))[0]
    h64 = chunk_cvs(cat(pre64, on64))[0]
    return digest_bytes(chunk_cvs(cat(h2, h64))[0])


# ---- the layouts the kernels read (data: one byte string per repetition, [R, n]) ----
def byte_rows(data):
    """[n_events][NQ] u32: repetition r's byte in word r // 4 at shift 24 - 8 (r % 4)"""
    data = np.asarray(data, np.uint8)
    R, n = data.shape
    assert R % 4 == 0
    d = data.T.reshape(n, R // 4, 4).astype(np.uint32)
    return np.ascontiguousarray((d[:, :, 0] << 24) | (d[:, :, 1] << 16) | (d[:, :, 2] << 8) | d[:, :, 3])


def bit_rows(bits):
    """bits [R, n] of 0 / 1 -> ([n_events][NQ / 2] u8, the byte strings hashed [R, n]): quad word q in byte q >> 1 at nibble shift
    4 (q & 1), repetition i4 of the quad at nibble bit 3 - i4; every bit is hashed as the byte 0x00 / 0xFF"""
    bits = np.asarray(bits, np.uint8)
    R, n = bits.shape
    assert R % 8 == 0 and bits.max(initial=0) <= 1
    b = bits.T.reshape(n, R // 8, 2, 4)  # [event][byte][q & 1][i4]
    nib = (b[..., 0] << 3) | (b[..., 1] << 2) | (b[..., 2] << 1) | b[..., 3]
    return np.ascontiguousarray(nib[:, :, 0] | (nib[:, :, 1] << 4)), bits * np.uint8(0xFF)


def contig_streams(data, stride_words, fill=0xEE):
    """[R][stride_words] u64 little-endian with data [R, 8 n_words] in front (the words behind it: `fill` bytes, never hashed)"""
    data = np.asarray(data, np.uint8)
    R, n = data.shape
    assert n % 8 == 0 and stride_words >= n // 8
    out = np.full((R, stride_words * 8), fill, np.uint8)
    out[:, :n] = data
    return np.ascontiguousarray(out.view("<u8"))


def scatter_quads(cvs, quads, fill=0xA5A5A5A5):
    """what a chunk kernel with a quad list leaves of cvs [n, R, 8] in a buffer of `fill` words: the listed quad words' repetitions"""
    out = np.full_like(cvs, fill)
    for q in quads:
        out[:, 4 * q:4 * q + 4] = cvs[:, 4 * q:4 * q + 4]
    return out


def load_official():
    """the official BLAKE3 C implementation as ROCm's libclang-cpp.so exports it (llvm_blake3_hasher_*; tests/golden/gen_golden.py took the
    known answers from it): blake3(data, n=32, seek=0) -> bytes.  Only the tests that tie this module to it call this."""
    lib = C.CDLL(os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "lib", "llvm", "lib", "libclang-cpp.so"))

    def blake3(data: bytes, n=32, seek=0) -> bytes:
        h = C.create_string_buffer(4096)
        lib.llvm_blake3_hasher_init(h)
        lib.llvm_blake3_hasher_update(h, data, C.c_size_t(len(data)))
        out = C.create_string_buffer(n)
        lib.llvm_blake3_hasher_finalize_seek(h, C.c_uint64(seek), out, C.c_size_t(n))
        return out.raw

    return blake3
