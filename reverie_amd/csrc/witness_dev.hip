// see witness_text.h
//
// Witness text read and written by kernels.  Reading is a stream compaction in two passes, with no workgroup waiting
// on another (no look-back, no spin):
//   1. count     a workgroup of 256 lanes takes a tile of 4096 bytes; the tile grid is laid on 16-byte-aligned addresses (tile 0
//                begins at the text pointer rounded down), so a text of any alignment is read with one 16-byte load per lane that
//                lies inside it; the lanes at the text's two ends go byte by byte (wt_lane_bytes).  The keep mask is SWAR on the four
//                words, the lane's count a population count; a wavefront reduction and four LDS words give the tile's count.
//   2. scan      scan_excl<SumU32> over the tile counts, in place; the total lands in a device word.
//   3. scatter   returns at once, uniformly, when the total exceeds the capacity.  Recomputes the mask; an exclusive prefix inside
//                the workgroup (a wavefront scan, the four wavefront totals through LDS); each lane drops its at most 16 values
//                into the tile's LDS image, which begins at the position modulo 16 its bytes have in d_bits; after the barrier the
//                image goes out: 16-byte stores for the aligned chunks that are wholly the tile's own, bytes at its two ends, where
//                a neighbour's bits share a chunk.  Neighbouring tiles write disjoint bytes; nothing is read, modified and rewritten.
//   4. marks     one wavefront per mark: the prefix of the mark's tile plus the kept bytes of that tile before the mark.
// Writing: every lane owns 16 output bytes on an aligned address, maps them back to bit indices (wt_write_range) and issues one
// 16-byte store; the lanes at the text's two ends go byte by byte.  A bit above 1 sets a flag word, one atomic per wavefront that
// saw one.
// All stores are plain vector stores.
#include "witness_text.h"

#include <algorithm>
#include <vector>

namespace rv {
namespace {
#include "compile_dev_prims.inc"
[[maybe_unused]] const auto unused_sort = &radix_sort;  // (the scans are all this file takes from the building blocks)
static_assert(TB * WT_LANE_BYTES == WT_TILE_BYTES && TB * 16 == WT_WRITE_TILE_BYTES, "the sizes rv_hook_witness_text_tiles reports");

constexpr uint32_t WAVES = TB / 64;
constexpr uint32_t IMAGE = 16 + WT_TILE_BYTES + 16;  // alignment, the tile's bits, the 16-byte readers' slack

// the lane's 16 bytes at c (16-byte aligned) of the text [lo, hi)
__device__ inline void lane_load(const uint8_t* c, const uint8_t* lo, const uint8_t* hi, uint32_t w[4]) {
    if (c >= lo && c + WT_LANE_BYTES <= hi) {
        const uint4 v = *reinterpret_cast<const uint4*>(c);
        w[0] = v.x, w[1] = v.y, w[2] = v.z, w[3] = v.w;
    } else if (c + WT_LANE_BYTES > lo && c < hi) {
        wt_lane_bytes(c, lo, hi, w);
    } else {
        w[0] = w[1] = w[2] = w[3] = 0;
    }
}
__device__ inline uint32_t wave_sum(uint32_t v) {
    for (int s = 32; s > 0; s >>= 1) v += __shfl_xor(v, s);
    return v;
}

// base: the text pointer rounded down to 16 bytes; tile t is base[t * 4096, (t + 1) * 4096)
__global__ __launch_bounds__(TB) void k_wt_count(const uint8_t* base, const uint8_t* lo, const uint8_t* hi, uint32_t* counts) {
    __shared__ uint32_t s_wave[WAVES];
    const uint8_t* c = base + (size_t)blockIdx.x * WT_TILE_BYTES + threadIdx.x * WT_LANE_BYTES;
    uint32_t w[4];
    lane_load(c, lo, hi, w);
    const uint32_t n = wave_sum(wt_lane_count(w));
    if ((threadIdx.x & 63u) == 0) s_wave[threadIdx.x >> 6] = n;
    __syncthreads();
    if (threadIdx.x == 0) counts[blockIdx.x] = s_wave[0] + s_wave[1] + s_wave[2] + s_wave[3];
}

__global__ __launch_bounds__(TB) void k_wt_scatter(const uint8_t* base, const uint8_t* lo, const uint8_t* hi, const uint32_t* offs, const uint32_t* total,
                                                   uint64_t cap, uint8_t* out) {
    __shared__ __attribute__((aligned(16))) uint8_t raw[IMAGE];
    __shared__ uint32_t s_wave[WAVES];
    if (*total > cap) return;
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint8_t* c = base + (size_t)blockIdx.x * WT_TILE_BYTES + threadIdx.x * WT_LANE_BYTES;
    uint32_t w[4];
    lane_load(c, lo, hi, w);
    const uint32_t mask = wt_keep_mask(w), mine = (uint32_t)__builtin_popcount(mask);
    uint32_t incl = mine;  // the wavefront's inclusive scan
    for (uint32_t d = 1; d < 64; d <<= 1) {
        const uint32_t t = __shfl_up(incl, d);
        if (lane >= d) incl += t;
    }
    if (lane == 63) s_wave[wave] = incl;
    __syncthreads();
    uint32_t before = incl - mine, count = 0;
    for (uint32_t k = 0; k < WAVES; k++) {
        if (k < wave) before += s_wave[k];
        count += s_wave[k];
    }
    // the tile's bytes: out[g0, g0 + count)
    const uint64_t g0 = offs[blockIdx.x];
    const uint32_t sh = (uint32_t)((uintptr_t)(out + g0) & 15u);
    wt_lane_values(w, mask, raw + sh + before);
    __syncthreads();
    const uint32_t span = sh + count;
    uint8_t* dst = out + g0 - sh;  // 16-byte aligned; only [sh, span) of it is this tile's to write
    for (uint32_t at = threadIdx.x * 16; at < span; at += TB * 16) {
        if (wt_chunk_whole(at, sh, span)) {
            *reinterpret_cast<uint4*>(dst + at) = *reinterpret_cast<const uint4*>(raw + at);
        } else {
            for (uint32_t k = 0; k < 16; k++)
                if (at + k >= sh && at + k < span) dst[at + k] = raw[at + k];
        }
    }
}

// mark m at text position p: offs[tile of p] + the kept bytes of that tile before p; shift = lo - base
__global__ __launch_bounds__(TB) void k_wt_marks(const uint8_t* base, const uint8_t* lo, uint32_t shift, const uint32_t* offs, const uint32_t* total,
                                                 uint32_t n_tiles, const uint64_t* marks, uint64_t n_marks, uint64_t* before) {
    const uint64_t m = (uint64_t)blockIdx.x * WAVES + (threadIdx.x >> 6);
    if (m >= n_marks) return;  // (uniform in the wavefront)
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t q = shift + marks[m];
    const uint32_t tile = (uint32_t)(q / WT_TILE_BYTES);
    uint32_t n = 0;
    if (tile < n_tiles) {
        const uint8_t* hi = lo + marks[m];
        for (uint32_t k = 0; k < WT_TILE_BYTES / (64 * WT_LANE_BYTES); k++) {
            const uint8_t* c = base + (size_t)tile * WT_TILE_BYTES + (k * 64 + lane) * WT_LANE_BYTES;
            uint32_t w[4];
            lane_load(c, lo, hi, w);
            n += wt_lane_count(w);
        }
    }
    n = wave_sum(n);
    if (lane == 0) before[m] = tile < n_tiles ? (uint64_t)offs[tile] + n : (uint64_t)*total;
}

// base: d_text rounded down to 16 bytes, shift = d_text - base; lane g owns base[g * 16, g * 16 + 16)
__global__ __launch_bounds__(TB) void k_wt_write(const uint8_t* bits, uint64_t n, uint64_t L, uint64_t len, uint8_t* base, uint32_t shift, uint32_t* flag) {
    const uint64_t a = ((uint64_t)blockIdx.x * TB + threadIdx.x) * 16;  // the lane's bytes are text bytes [a - shift, a - shift + 16)
    uint64_t j0, j1;
    wt_lane_range(a, shift, len, &j0, &j1);
    bool bad = false;
    if (j0 < j1) {
        if (j1 - j0 == 16) {
            __attribute__((aligned(16))) uint8_t v[16];
            bad = wt_write_range(j0, j1, L, n, bits, v);
            *reinterpret_cast<uint4*>(base + a) = *reinterpret_cast<const uint4*>(v);
        } else {
            bad = wt_write_range(j0, j1, L, n, bits, base + shift + j0);
        }
    }
    if (__any(bad) && (threadIdx.x & 63u) == 0) atomicOr(flag, 1u);
}

}  // namespace

int witness_parse_device(hipStream_t st, const DevAlloc& A, const uint8_t* d_text, size_t len, uint8_t* d_bits, uint64_t cap, const uint64_t* d_marks,
                         size_t n_marks, uint64_t* bits_before, WitnessParse* res) {
    *res = WitnessParse{};
    if (!len) {  // (no tile at all)
        for (size_t m = 0; m < n_marks; m++) bits_before[m] = 0;
        res->written = d_bits != nullptr;
        return RV_OK;
    }
    Scratch S(A, st);
    const uint32_t shift = (uint32_t)((uintptr_t)d_text & 15u);
    const uint8_t* base = d_text - shift;
    const uint32_t n_tiles = (uint32_t)(((uint64_t)shift + len + WT_TILE_BYTES - 1) / WT_TILE_BYTES);
    uint32_t* counts = S.get<uint32_t>(n_tiles);
    uint32_t* total = S.get<uint32_t>(1);
    uint64_t* before = n_marks ? S.get<uint64_t>(n_marks) : nullptr;
    CDNEED(counts && total && (before || !n_marks));

    k_wt_count<<<n_tiles, TB, 0, st>>>(base, d_text, d_text + len, counts);
    CDCHK(hipGetLastError());
    CDCHK((scan_excl<uint32_t, SumU32>(S, st, counts, counts, n_tiles, total)));  // (len < 2^32: no sum wraps)
    if (d_bits) k_wt_scatter<<<n_tiles, TB, 0, st>>>(base, d_text, d_text + len, counts, total, cap, d_bits);
    if (n_marks) k_wt_marks<<<blocks(n_marks, WAVES), TB, 0, st>>>(base, d_text, shift, counts, total, n_tiles, d_marks, n_marks, before);
    CDCHK(hipGetLastError());
    std::vector<uint32_t> h(1);
    CDCHK(fetch(st, h, total));
    if (n_marks) CDCHK(hipMemcpyAsync(bits_before, before, n_marks * sizeof(uint64_t), hipMemcpyDeviceToHost, st));
    CDCHK(hipStreamSynchronize(st));
    res->bits = h[0];
    res->written = d_bits && res->bits <= cap;
    return RV_OK;
}

int witness_write_device(hipStream_t st, const DevAlloc& A, const uint8_t* d_bits, size_t n, uint64_t line_bits, uint8_t* d_text, bool* bad) {
    *bad = false;
    const uint64_t len = wt_text_len(n, line_bits);
    if (!len) return RV_OK;
    Scratch S(A, st);
    uint32_t* flag = S.get<uint32_t>(1);
    CDNEED(flag);
    const uint32_t shift = (uint32_t)((uintptr_t)d_text & 15u);
    CDCHK(hipMemsetAsync(flag, 0, sizeof(uint32_t), st));
    k_wt_write<<<blocks(shift + len, WT_WRITE_TILE_BYTES), TB, 0, st>>>(d_bits, n, wt_line(n, line_bits), len, d_text - shift, shift, flag);
    CDCHK(hipGetLastError());
    std::vector<uint32_t> h(1);
    CDCHK(fetch(st, h, flag));
    CDCHK(hipStreamSynchronize(st));
    *bad = h[0] != 0;
    return RV_OK;
}
#undef CDCHK
#undef CDNEED

}  // namespace rv
