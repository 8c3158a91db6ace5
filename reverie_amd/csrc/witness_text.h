// Witness text -- '0' and '1' are bits, every other byte is skipped -- read and written on the host (rv_witness_parse,
// rv_witness_write: witness.cpp), on the GPU (witness_dev.hip) and in windows (rv_witness_reader_*).  The rule is in
// include/reverie_amd.h, the stages in DESIGN §21 and at the head of witness_dev.hip.
//
// WHICH BYTES OF A LANE ARE KEPT (wt_keep_mask), WHAT A KEPT BYTE IS WORTH (wt_bit_value) AND WHICH BIT AN OUTPUT BYTE SHOWS (wt_map)
// are decided here and nowhere else: the host functions, the kernels and the CPU model of tests/witness_text_model.cpp all call
// these functions.
//
// Everything up to the `rv` device entry points at the end is plain C++ (no HIP header is needed: the CPU model compiles it with g++).
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "../../include/reverie_amd.h"

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define WT_HD __host__ __device__
#else
#define WT_HD
#endif

namespace rv {

// bytes of text one workgroup of the parse kernels covers (256 lanes of 16 bytes), tiles per workgroup, and bytes of text one
// workgroup of the writer stores (rv_hook_witness_text_tiles reports the first times the second, and the third)
constexpr uint32_t WT_LANE_BYTES = 16;
constexpr uint32_t WT_TILE_BYTES = 4096;
constexpr uint32_t WT_WG_TILES = 1;
constexpr uint32_t WT_WRITE_TILE_BYTES = 4096;

// ---- reading: a lane's 16 bytes as four little-endian words (a byte outside the text is 0, which is no bit) ----
WT_HD inline bool wt_is_bit(uint32_t b) { return (b ^ 0x30u) <= 1u; }
WT_HD inline uint32_t wt_bit_value(uint32_t b) { return b & 1u; }
WT_HD inline uint32_t wt_bit_values(uint32_t w) { return w & 0x01010101u; }  // of a word whose four bytes are all kept
// bit 8k+7 of the result = byte k of w is '0' or '1' (SWAR: a byte is kept iff (b ^ 0x30) & 0xFE == 0)
WT_HD inline uint32_t wt_keep_word(uint32_t w) {
    const uint32_t y = (w ^ 0x30303030u) & 0xFEFEFEFEu;
    const uint32_t nz = ((y & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | y;  // bit 7 of each byte: the byte of y is not 0 (no carry leaves a byte)
    return ~nz & 0x80808080u;
}
// bit k of the result = byte k of the lane is kept; its population count is the lane's count
WT_HD inline uint32_t wt_keep_mask(const uint32_t w[4]) {
    uint32_t mask = 0;
    for (int q = 0; q < 4; q++) {
        const uint32_t m = wt_keep_word(w[q]) >> 7;  // bits 0, 8, 16, 24
        mask |= ((m | m >> 7 | m >> 14 | m >> 21) & 0xFu) << (4 * q);
    }
    return mask;
}
WT_HD inline uint32_t wt_lane_count(const uint32_t w[4]) {
    return (uint32_t)(__builtin_popcount(wt_keep_word(w[0])) + __builtin_popcount(wt_keep_word(w[1])) + __builtin_popcount(wt_keep_word(w[2])) +
                      __builtin_popcount(wt_keep_word(w[3])));
}
// the bytes of c[0, 16) that lie in [lo, hi), one at a time (an edge lane; a lane that lies inside takes one 16-byte load instead)
WT_HD inline void wt_lane_bytes(const uint8_t* c, const uint8_t* lo, const uint8_t* hi, uint32_t w[4]) {
    w[0] = w[1] = w[2] = w[3] = 0;
    const int from = c < lo ? (int)(lo - c) : 0, to = hi - c < 16 ? (int)(hi - c) : 16;
    for (int k = from; k < to; k++) w[k >> 2] |= (uint32_t)c[k] << (8 * (k & 3));
}
// the lane's kept values, in order, to dst[0, popcount(mask))
WT_HD inline void wt_lane_values(const uint32_t w[4], uint32_t mask, uint8_t* dst) {
    while (mask) {
        const int k = __builtin_ctz(mask);
        mask &= mask - 1;
        *dst++ = (uint8_t)wt_bit_value(w[k >> 2] >> (8 * (k & 3)));
    }
}

// the tile's LDS image holds its bits at image[sh, span), sh = the position modulo 16 of its first bit in d_bits: the chunk
// image[at, at + 16) goes out with one 16-byte store iff all 16 bytes are the tile's own (else byte by byte, the own ones only)
WT_HD inline bool wt_chunk_whole(uint32_t at, uint32_t sh, uint32_t span) { return at >= sh && at + 16 <= span; }

// ---- writing: output byte j of n bits in lines of L bits (L = wt_line(n, line_bits): one line is a line of n bits) ----
WT_HD inline uint64_t wt_line(uint64_t n, uint64_t line_bits) { return line_bits && line_bits < n ? line_bits : n; }
WT_HD inline uint64_t wt_text_len(uint64_t n, uint64_t line_bits) {
    if (!n) return 0;
    const uint64_t L = wt_line(n, line_bits);
    return n + (n / L + (n % L ? 1 : 0));
}
// byte j of the text (j < wt_text_len): a line feed (true), or bit *i (false)
WT_HD inline bool wt_map(uint64_t j, uint64_t L, uint64_t n, uint64_t* i) {
    const uint64_t g = j / (L + 1), r = j % (L + 1);
    *i = g * L + r;
    return r == L || *i == n;
}
// bytes [j0, j1) of the text to out[0, j1 - j0): one division, then a walk.  -> a bit above 1 was met (its byte is then unspecified)
WT_HD inline bool wt_write_range(uint64_t j0, uint64_t j1, uint64_t L, uint64_t n, const uint8_t* bits, uint8_t* out) {
    if (j0 >= j1) return false;
    uint64_t i;
    (void)wt_map(j0, L, n, &i);
    uint64_t r = j0 % (L + 1);
    uint32_t bad = 0;
    for (uint64_t j = j0; j < j1; j++) {
        if (r == L || i == n) {
            out[j - j0] = '\n';
            r = 0;  // (the next byte opens a line; i already names its first bit)
        } else {
            const uint32_t b = bits[i];
            bad |= b;
            out[j - j0] = (uint8_t)('0' + (b & 1u));
            i++, r++;
        }
    }
    return bad > 1;
}

// the writer's lane whose 16 bytes begin a bytes behind the text pointer rounded down to 16 (shift = pointer & 15): it owns text
// bytes [j0, j1) of len; all 16 (one 16-byte store) iff j1 - j0 == 16
WT_HD inline void wt_lane_range(uint64_t a, uint32_t shift, uint64_t len, uint64_t* j0, uint64_t* j1) {
    *j0 = a > shift ? a - shift : 0;
    *j1 = a + 16 - shift < len ? a + 16 - shift : len;
}

}  // namespace rv

#if defined(__HIPCC__)
#include "compile_dev.h"

namespace rv {

struct WitnessParse {
    uint64_t bits = 0;     // '0' / '1' bytes of the text
    bool written = false;  // the bits were written (a destination was given and the capacity sufficed)
};

// d_text[0, len): the text in device memory (any alignment, len < 2^32).  d_bits / cap: where the bits go (null: nowhere); they are
// written only when all of them fit -- decided on the device, so the stream is synchronised once, at the end.  d_marks (device
// memory, n_marks ascending positions <= len; may be null): bits_before[m] (host) = the bits of d_text[0, d_marks[m]).  Work memory
// (4 bytes per 4096 bytes of text, the scan's sums, 8 bytes per mark) from A, given back before the call returns.
// RV_OK (res filled), RV_E_NOMEM or RV_E_DEVICE.
int witness_parse_device(hipStream_t st, const DevAlloc& A, const uint8_t* d_text, size_t len, uint8_t* d_bits, uint64_t cap, const uint64_t* d_marks,
                         size_t n_marks, uint64_t* bits_before, WitnessParse* res);

// d_bits[0, n) -> d_text[0, wt_text_len(n, line_bits)) (both < 2^32; the caller has checked the room).  *bad: a byte above 1 was met.
int witness_write_device(hipStream_t st, const DevAlloc& A, const uint8_t* d_bits, size_t n, uint64_t line_bits, uint8_t* d_text, bool* bad);

}  // namespace rv
#endif
