// see piece_sums.h
//
// One thread per op with a stride loop over the piece (blockIdx.y = piece, blockIdx.x = the workgroups that share it).  An op is
// three aligned 64-bit words; every rule below is the host loop's, bad opcodes and domains included (they count as whatever the host
// comparisons make of them: the compiler reports the error, not this kernel).  The ten sums go through the wavefront (shuffles),
// the workgroup (LDS) and one 64-bit atomic add each per workgroup: integer sums, so the order of arrival does not matter.
#include "piece_sums.h"

#include <algorithm>

namespace rv {

namespace {

constexpr int TB = 256;  // threads per workgroup
constexpr int WAVE = 64;
constexpr int OPS_PER_THREAD = 8;    // what a thread of a full-size grid sums before the reduction
constexpr uint32_t MAX_GROUPS = 64;  // workgroups per piece at most (64 x 256 x 8 = 2^17 ops per trip of the stride loop)
constexpr uint32_t MAX_GRID_Y = 65535;

__global__ __launch_bounds__(TB) void k_piece_sums(const rv_op* __restrict__ ops, const uint64_t* __restrict__ cut, uint64_t piece0, uint64_t first_index,
                                                   PieceSums* __restrict__ sums) {
    const uint64_t piece = piece0 + blockIdx.y;
    const uint64_t lo = cut[piece], hi = cut[piece + 1];
    uint64_t acc[PIECE_SUM_WORDS];
    for (int k = 0; k < PIECE_SUM_WORDS; k++) acc[k] = 0;
    for (uint64_t i = lo + (uint64_t)blockIdx.x * TB + threadIdx.x; i < hi; i += (uint64_t)gridDim.x * TB) {
        const uint64_t* p = (const uint64_t*)(ops + i);
        const uint64_t w0 = p[0], w1 = p[1], w2 = p[2];
        const uint32_t domain = (uint32_t)(w0 & 0xFF), opcode = (uint32_t)(w0 >> 8) & 0xFF;
        // ops_digest: domain, opcode and dst (not the reserved half-word), then a | b << 32, then imm
        uint64_t h = (first_index + i) * 0x9E3779B97F4A7C15ull;
        const uint64_t w[3] = {w0 & 0xFFFFFFFF0000FFFFull, w1, w2};
        for (int k = 0; k < 3; k++) {
            h ^= w[k] + 0x9E3779B97F4A7C15ull + (h << 6) + (h >> 2);
            h *= 0xFF51AFD7ED558CCDull;
            h ^= h >> 29;
        }
        acc[0] += h;
        const bool one = opcode == RV_OP_INPUT || opcode == RV_OP_RANDOM, mul = opcode == RV_OP_MUL, az = opcode == RV_OP_ASSERTZERO;
        if (domain == RV_DOM_GF2) {
            acc[1] += one ? 1 : (mul ? 2 : 0);
            acc[3] += opcode == RV_OP_INPUT;
            acc[4] += mul || az;
            acc[5] += mul;
        } else {
            acc[8] += 1;
            if (domain == RV_DOM_Z64) {
                acc[2] += one ? 1 : (mul ? 2 : 0);
                acc[6] += opcode == RV_OP_INPUT ? 1 : ((mul || az) ? 8 : 0);
                acc[7] += mul;
            } else if (domain != RV_DOM_SIZEHINT) {
                acc[9] += 1;
            }
            if (domain == RV_DOM_B2A) {  // 64 fresh masks + 63 Mul, one Z64 mask
                acc[1] += 64 + 63 * 2;
                acc[2] += 1;
                acc[4] += 63 + 64;
                acc[5] += 63;
                acc[7] += 1;
            }
        }
    }
    __shared__ uint64_t sh[TB / WAVE][PIECE_SUM_WORDS];
    const uint32_t lane = threadIdx.x % WAVE, wave = threadIdx.x / WAVE;
    for (int k = 0; k < PIECE_SUM_WORDS; k++) {
        unsigned long long v = acc[k];
        for (int d = WAVE / 2; d > 0; d >>= 1) v += __shfl_down(v, d, WAVE);
        if (lane == 0) sh[wave][k] = v;
    }
    __syncthreads();
    if (threadIdx.x < PIECE_SUM_WORDS) {
        unsigned long long v = 0;
        for (int wv = 0; wv < TB / WAVE; wv++) v += sh[wv][threadIdx.x];
        if (v) atomicAdd((unsigned long long*)&sums[piece] + threadIdx.x, v);
    }
}

// wit_digest's sum for proof blockIdx.y: item i < n2 is a GF(2) byte (only bit 0 counts), item n2 + j a Z64 word; each keyed by its
// input ordinal (64-bit: a long stream's ordinals pass 2^32).  The reduction is k_piece_sums': wavefront, LDS, one atomic add.
__global__ __launch_bounds__(TB) void k_wit_sums(const uint8_t* __restrict__ w2, uint64_t stride2, uint64_t n2, uint64_t first2,
                                                 const uint64_t* __restrict__ w64, uint64_t stride64, uint64_t n64, uint64_t first64, WitSumsAcc A) {
    const uint8_t* p2 = w2 + (uint64_t)blockIdx.y * stride2;      // (not dereferenced when n2 == 0)
    const uint64_t* p64 = w64 + (uint64_t)blockIdx.y * stride64;  // (... n64 == 0)
    auto mix = [](uint64_t pos, uint64_t x) {
        uint64_t h = pos * 0x9E3779B97F4A7C15ull;
        h ^= x + 0x9E3779B97F4A7C15ull + (h << 6) + (h >> 2);
        h *= 0xFF51AFD7ED558CCDull;
        return h ^ (h >> 29);
    };
    unsigned long long v = 0;
    const uint64_t total = n2 + n64;
    for (uint64_t i = (uint64_t)blockIdx.x * TB + threadIdx.x; i < total; i += (uint64_t)gridDim.x * TB)
        v += i < n2 ? mix(2 * (first2 + i), p2[i] & 1u) : mix(2 * (first64 + (i - n2)) + 1, p64[i - n2]);
    __shared__ uint64_t sh[TB / WAVE];
    for (int d = WAVE / 2; d > 0; d >>= 1) v += __shfl_down(v, d, WAVE);
    if (threadIdx.x % WAVE == 0) sh[threadIdx.x / WAVE] = v;
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned long long s = 0;
        for (int wv = 0; wv < TB / WAVE; wv++) s += sh[wv];
        if (s) atomicAdd((unsigned long long*)A.acc[blockIdx.y], s);
    }
}

}  // namespace

void launch_wit_sums(hipStream_t st, const uint8_t* d_w2, uint64_t stride2, uint64_t n2, uint64_t first2, const uint64_t* d_w64, uint64_t stride64,
                     uint64_t n64, uint64_t first64, uint64_t* const* acc, size_t n_proofs) {
    if (!n_proofs || !(n2 + n64)) return;
    const size_t per_group = (size_t)TB * 4;
    const uint32_t gx = (uint32_t)std::min<size_t>(std::max<size_t>((n2 + n64 + per_group - 1) / per_group, 1), MAX_GROUPS);
    for (size_t b0 = 0; b0 < n_proofs; b0 += WitSumsAcc::MAX) {
        WitSumsAcc A{};
        const uint32_t nb = (uint32_t)std::min<size_t>(n_proofs - b0, WitSumsAcc::MAX);
        for (uint32_t b = 0; b < nb; b++) A.acc[b] = acc[b0 + b];
        hipLaunchKernelGGL(k_wit_sums, dim3(gx, nb), dim3(TB), 0, st, d_w2 + b0 * stride2, stride2, n2, first2, d_w64 + b0 * stride64, stride64, n64, first64, A);
    }
}

void launch_piece_sums(hipStream_t st, const rv_op* d_ops, const uint64_t* d_cut, size_t n_pieces, size_t max_piece, uint64_t first_index,
                       PieceSums* d_sums) {
    if (!n_pieces) return;
    (void)hipMemsetAsync(d_sums, 0, n_pieces * sizeof(PieceSums), st);
    const size_t per_group = (size_t)TB * OPS_PER_THREAD;
    const uint32_t gx = (uint32_t)std::min<size_t>(std::max<size_t>((max_piece + per_group - 1) / per_group, 1), MAX_GROUPS);
    for (size_t p0 = 0; p0 < n_pieces; p0 += MAX_GRID_Y) {
        const uint32_t gy = (uint32_t)std::min<size_t>(n_pieces - p0, MAX_GRID_Y);
        hipLaunchKernelGGL(k_piece_sums, dim3(gx, gy), dim3(TB), 0, st, d_ops, d_cut, (uint64_t)p0, first_index, d_sums);
    }
}

}  // namespace rv
