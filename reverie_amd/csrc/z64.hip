// Z64 ring interpreter, transcript hashing and openings for gfx950.
//
// Replaces (all under /root/reference/src/):
//   algebra/z64/{share,recon,domain}.rs       wrapping u64 arithmetic per (rep, player)
//   interpreter/single.rs:25-157              Instance::step / op_mul instantiated at Z64
//   interpreter/combine.rs:19-36,132-219      recon_gf2_to_z64 and the Z64 half of B2A
//   transcript/{prover,verifier/*}.rs         the same transcript rules as GF(2)
//
// Lane mapping: one lane = two players of one repetition (16-byte accesses), 4 adjacent lanes = one
// repetition; reconstruct = a local add + 2-step shuffle-add inside the 4-lane group.  A gate occupies
// R*4 lanes (16 wavefronts at R = 256).
#include <algorithm>
#include <atomic>

#include "b3.h"
#include "internal.h"
#include "launch.h"

namespace rv {

__device__ __forceinline__ uint64_t shfl_xor64(uint64_t v, int m) {
    const uint32_t lo = __shfl_xor((uint32_t)v, m), hi = __shfl_xor((uint32_t)(v >> 32), m);
    return ((uint64_t)hi << 32) | lo;
}
__device__ __forceinline__ uint32_t recon32_(uint32_t t) {
    t ^= t >> 4;
    t ^= t >> 2;
    t ^= t >> 1;
    t &= 0x01010101u;
    return (t << 8) - t;
}

// Two players per lane: every row access is a 16-byte load/store (twice the bytes in flight per wavefront of the
// first, one-u64-per-lane version, which ran at 2.7 TB/s), a gate occupies R*4 lanes and the player sum is one local
// add plus two shuffle steps inside the 4-lane group of a repetition.
struct U2 {
    uint64_t x, y;
};
__device__ __forceinline__ U2 ld2(const uint64_t* p) {
    const ulonglong2 v = *(const ulonglong2*)p;
    return U2{v.x, v.y};
}
__device__ __forceinline__ void st2(uint64_t* p, U2 v) { *(ulonglong2*)p = make_ulonglong2(v.x, v.y); }
// transcript words are only 8-byte aligned (an odd number of 8-byte events may precede a 64-byte one)
__device__ __forceinline__ void st2_unaligned(uint64_t* p, U2 v) {
    p[0] = v.x;
    p[1] = v.y;
}
// DomainZ64::reconstruct (z64/domain.rs:53-61): wrapping sum over the 8 players
__device__ __forceinline__ uint64_t sum8(U2 v) {
    uint64_t t = v.x + v.y;
    t += shfl_xor64(t, 1);
    t += shfl_xor64(t, 2);
    return t;
}

// parity hook for DomainZ64::reconstruct (z64/domain.rs:53-61) on ShareZ64 values ([8 reps][8 players] u64 each): the
// interpreter's own lane mapping (two players per lane, four lanes per repetition) and its sum8
__global__ void k_hook_recon_z64(const uint64_t* __restrict__ shares, uint64_t n_reps_total, uint64_t* __restrict__ out) {
    const uint64_t tid = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const uint64_t r = tid >> 2;
    const U2 v = r < n_reps_total ? ld2(shares + 2 * tid) : U2{0, 0};
    const uint64_t s = sum8(v);
    if (r < n_reps_total && (tid & 3) == 0) out[r] = s;
}
void launch_hook_recon_z64(hipStream_t st, const uint64_t* d_shares, uint64_t n, uint64_t* d_out) {
    const uint64_t lanes = n * 8 * 4;
    if (n) hipLaunchKernelGGL(k_hook_recon_z64, dim3((unsigned)((lanes + 255) / 256)), dim3(256), 0, st, d_shares, n * 8, d_out);
}

template <int MODE>
__global__ __launch_bounds__(256) void k_interp64(const Gate64* __restrict__ gates, uint32_t lo, uint32_t hi, Interp64Params p) {
#include "z64_interp.inc"
}

// Batched proofs of one circuit (rv_prove_batch / rv_verify_batch): blockIdx.y selects the proof, whose buffers come from a
// device array of Interp64Params; the level's gate range is shared, so one launch per level serves the whole batch.  The body
// sees its own proof's grid only (gridDim.x workgroups): the worker decomposition is that of k_interp64.
template <int MODE>
__global__ __launch_bounds__(256) void k_interp64_b(const Gate64* __restrict__ gates, uint32_t lo, uint32_t hi, const Interp64Params* __restrict__ pp) {
    const Interp64Params p = pp[blockIdx.y];
#include "z64_interp.inc"
}

static std::atomic<uint64_t> g_interp64_launches[IX64_COUNT][2];
void count_interp64_launch(int exec, bool verify) { g_interp64_launches[exec][verify ? 1 : 0].fetch_add(1, std::memory_order_relaxed); }
void interp64_launch_counts(uint64_t out[][2], bool reset) {
    for (int e = 0; e < IX64_COUNT; e++)
        for (int m = 0; m < 2; m++)
            out[e][m] = reset ? g_interp64_launches[e][m].exchange(0, std::memory_order_relaxed) : g_interp64_launches[e][m].load(std::memory_order_relaxed);
}

void launch_interp64(hipStream_t st, int mode, const Gate64* d_gates, uint32_t lo, uint32_t hi, const Interp64Params& p) {
    if (hi <= lo) return;
    count_interp64_launch(IX64_INTERP, mode != MODE_PROVE);
    const uint64_t S2 = (uint64_t)p.R * 4;  // lanes per gate
    const uint64_t want = (uint64_t)(hi - lo) * S2;
    uint64_t blocks = (want + 255) / 256;
    const uint64_t cap = ((uint64_t)8192 * 256 / S2) * S2 / 256;  // whole workers only
    if (blocks > cap) blocks = cap;
    if (mode == MODE_PROVE)
        hipLaunchKernelGGL(k_interp64<MODE_PROVE>, dim3((unsigned)blocks), dim3(256), 0, st, d_gates, lo, hi, p);
    else
        hipLaunchKernelGGL(k_interp64<MODE_VERIFY>, dim3((unsigned)blocks), dim3(256), 0, st, d_gates, lo, hi, p);
}

// rv_prove_batch / rv_verify_batch: one level of `batch` whole proofs (R = 256).  A proof's workers are capped so that the
// whole launch keeps to the single launch's 8 192 workgroups: a level of a few gates fills the chip only through the batch.
void launch_interp64_batched(hipStream_t st, int mode, const Gate64* d_gates, uint32_t lo, uint32_t hi, const Interp64Params* d_pp, uint32_t batch) {
    if (hi <= lo || !batch) return;
    count_interp64_launch(IX64_INTERP_B, mode != MODE_PROVE);
    const uint64_t S2 = (uint64_t)RV_TOTAL_REPS * 4;  // lanes per gate
    const uint64_t bpw = S2 / 256;                     // workgroups per worker
    uint64_t workers = hi - lo;
    const uint64_t cap = std::max<uint64_t>((uint64_t)8192 / bpw / batch, 1);
    if (workers > cap) workers = cap;
    if (mode == MODE_PROVE)
        hipLaunchKernelGGL(k_interp64_b<MODE_PROVE>, dim3((unsigned)(workers * bpw), batch), dim3(256), 0, st, d_gates, lo, hi, d_pp);
    else
        hipLaunchKernelGGL(k_interp64_b<MODE_VERIFY>, dim3((unsigned)(workers * bpw), batch), dim3(256), 0, st, d_gates, lo, hi, d_pp);
}

// ---- BLAKE3 over R contiguous little-endian streams: thread = (chunk, rep), chunk fastest ----
// Adjacent lanes hash adjacent 1 KiB chunks of the SAME stream, so a wavefront walks one contiguous 64 KiB region
// (the first version put the repetitions of one chunk in adjacent lanes: 64 MB apart, every 16-byte load a different
// DRAM page, 1.2 TB/s).  A lane fetches a whole 128-byte line (two blocks, eight 16-byte loads issued together) and
// then runs the two dependent compressions, so each line crosses L2 -> L1 once instead of eight times.
// stride_bytes: distance between two repetitions' streams (>= n_bytes; the streaming prover hashes a prefix of each);
// chunk_base / root_ok: see B_k_b3_chunks
struct B_k_b3_chunks_contig {
    __device__ __forceinline__ void operator()(const uint32_t* __restrict__ streams, uint64_t stride_bytes, uint64_t n_bytes, uint32_t R,
                                               uint64_t n_chunks, uint32_t* __restrict__ cvs, uint64_t chunk_base, uint32_t root_ok) const {
    const uint64_t tid = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const uint64_t c = tid % n_chunks;
    const uint32_t r = (uint32_t)(tid / n_chunks);
    if (r >= R) return;
    const uint64_t b0 = c * 1024;
    const uint64_t len = (n_bytes - b0 < 1024) ? (n_bytes - b0) : 1024;
    const uint32_t nblk = len == 0 ? 1 : (uint32_t)((len + 63) / 64);
    const uint32_t* src = streams + ((size_t)r * stride_bytes + b0) / 4;
    uint32_t cv[8];
    b3::iv(cv);
    uint32_t b = 0;
    if (len == 1024 && n_chunks > 1) {  // the common case: 16 full blocks, two per step
        for (; b < 16; b += 2) {
            const uint4* s4 = (const uint4*)(src + 16 * b);
            uint4 v[8];
#pragma unroll
            for (int k = 0; k < 8; k++) v[k] = s4[k];
#pragma unroll
            for (int h = 0; h < 2; h++) {
                uint32_t m[16], o[8];
#pragma unroll
                for (int k = 0; k < 4; k++) {
                    m[4 * k] = v[4 * h + k].x;
                    m[4 * k + 1] = v[4 * h + k].y;
                    m[4 * k + 2] = v[4 * h + k].z;
                    m[4 * k + 3] = v[4 * h + k].w;
                }
                const uint32_t flags = (b + h == 0 ? b3::CHUNK_START : 0u) | (b + h == 15 ? b3::CHUNK_END : 0u);
                b3::compress<false>(cv, m, c + chunk_base, 64, flags, o);
#pragma unroll
                for (int k = 0; k < 8; k++) cv[k] = o[k];
            }
        }
    }
    for (; b < nblk; b++) {
        const uint32_t blen = (b + 1 < nblk) ? 64u : (uint32_t)(len - 64ull * b);
        uint32_t flags = (b == 0 ? b3::CHUNK_START : 0u) | (b + 1 == nblk ? b3::CHUNK_END : 0u);
        if (b + 1 == nblk && n_chunks == 1 && root_ok) flags |= b3::ROOT;
        uint32_t m[16];
#pragma unroll
        for (int k = 0; k < 16; k++) {
            uint32_t w = (4u * k < blen) ? src[16 * b + k] : 0u;
            if (4u * k < blen && 4u * k + 4 > blen) w &= (1u << (8 * (blen - 4u * k))) - 1u;  // byte streams: the last word may be partial
            m[k] = w;
        }
        uint32_t o[8];
        b3::compress<false>(cv, m, c + chunk_base, blen, flags, o);
#pragma unroll
        for (int k = 0; k < 8; k++) cv[k] = o[k];
    }
    uint32_t* dst = cvs + ((size_t)c * R + r) * 8;
#pragma unroll
    for (int k = 0; k < 8; k++) dst[k] = cv[k];
}
};
__global__ __launch_bounds__(256) void k_b3_chunks_contig(const uint32_t* __restrict__ streams, uint64_t stride_bytes, uint64_t n_bytes, uint32_t R,
                                                          uint64_t n_chunks, uint32_t* __restrict__ cvs, uint64_t chunk_base, uint32_t root_ok) {
    B_k_b3_chunks_contig{}(streams, stride_bytes, n_bytes, R, n_chunks, cvs, chunk_base, root_ok);
}

void launch_b3_contig_chunks(hipStream_t st, const uint64_t* d_streams, uint64_t stride_words, uint64_t n_words, uint32_t R, uint32_t* d_cv,
                             uint64_t chunk_base, uint32_t root_ok) {
    const uint64_t n_bytes = n_words * 8;
    const uint64_t n = n_bytes == 0 ? 1 : (n_bytes + 1023) / 1024;
    const uint64_t threads = n * R;
    launch<B_k_b3_chunks_contig, 256>(k_b3_chunks_contig, st, dim3((unsigned)((threads + 255) / 256)), dim3(256), (const uint32_t*)d_streams,
                                      stride_words * 8, n_bytes, R, n, d_cv, chunk_base, root_ok);
}

uint32_t launch_b3_contig(hipStream_t st, const uint64_t* d_streams, uint64_t n_words, uint32_t R, uint32_t* d_cv_a, uint32_t* d_cv_b,
                      uint32_t* d_digest) {
    const uint64_t n_bytes = n_words * 8;
    const uint64_t n = n_bytes == 0 ? 1 : (n_bytes + 1023) / 1024;
    launch_b3_contig_chunks(st, d_streams, n_words, n_words, R, d_cv_a, 0, 1);
    return 1 + b3_reduce_tree(st, d_cv_a, d_cv_b, n, R, d_digest);  // launches
}

// ---- openings: 8 bytes LE per item (z64/share.rs:36-49, z64/recon.rs:45-66) ----
struct B_k_extract64 {
    __device__ __forceinline__ void operator()(const uint64_t* __restrict__ stream, uint64_t stride_words, const uint64_t* __restrict__ offs,
                                               uint64_t n_items, int add_omit, uint32_t R, const uint8_t* __restrict__ omit,
                                               const uint64_t* __restrict__ dst_off, uint8_t* __restrict__ out) const {
    const uint64_t tid = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const uint64_t it = tid % n_items;
    const uint32_t r = (uint32_t)(tid / n_items);
    if (r >= R) return;
    const uint32_t om = omit[r];
    if (om >= 8) return;
    const uint64_t off = (offs ? offs[it] : it) + (add_omit ? om : 0);
    const uint64_t v = stream[(size_t)r * stride_words + off];
    uint8_t* d = out + dst_off[r] + 8 * it;
#pragma unroll
    for (int i = 0; i < 8; i++) d[i] = (uint8_t)(v >> (8 * i));
}
};
__global__ void k_extract64(const uint64_t* __restrict__ stream, uint64_t stride_words, const uint64_t* __restrict__ offs,
                            uint64_t n_items, int add_omit, uint32_t R, const uint8_t* __restrict__ omit,
                            const uint64_t* __restrict__ dst_off, uint8_t* __restrict__ out) {
    B_k_extract64{}(stream, stride_words, offs, n_items, add_omit, R, omit, dst_off, out);
}

// the same over the opened repetitions only (ol: the shard's OnlineList in device memory): thread = (rank among the opened, item) --
// 40 x n_items threads instead of R x n_items of which 216 in 256 returned at once (10^6-MUL circuit: opening phase 1.06 -> 0.75 ms)
struct B_k_extract64_ol {
    __device__ __forceinline__ void operator()(const uint64_t* __restrict__ stream, uint64_t stride_words, const uint64_t* __restrict__ offs,
                                               uint64_t n_items, int add_omit, const OnlineList* __restrict__ ol, const uint8_t* __restrict__ omit,
                                               const uint64_t* __restrict__ dst_off, uint8_t* __restrict__ out, uint32_t rep_min) const {
    const uint64_t tid = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const uint64_t it = tid % n_items;
    const uint32_t k = (uint32_t)(tid / n_items);
    if (k >= ol->n || k >= RV_ONLINE_REPS) return;
    const uint32_t r = ol->rep[k];
    if (r < rep_min) return;  // (Z64 early corrections: the host has this repetition's vector already)
    const uint32_t om = omit[r];
    const uint64_t off = (offs ? offs[it] : it) + (add_omit ? om : 0);
    const uint64_t v = stream[(size_t)r * stride_words + off];
    uint8_t* d = out + dst_off[r] + 8 * it;
#pragma unroll
    for (int i = 0; i < 8; i++) d[i] = (uint8_t)(v >> (8 * i));
}
};
__global__ void k_extract64_ol(const uint64_t* __restrict__ stream, uint64_t stride_words, const uint64_t* __restrict__ offs,
                               uint64_t n_items, int add_omit, const OnlineList* __restrict__ ol, const uint8_t* __restrict__ omit,
                               const uint64_t* __restrict__ dst_off, uint8_t* __restrict__ out, uint32_t rep_min) {
    B_k_extract64_ol{}(stream, stride_words, offs, n_items, add_omit, ol, omit, dst_off, out, rep_min);
}

void launch_extract64(hipStream_t st, const uint64_t* d_stream, uint64_t stride_words, const uint64_t* d_offs, uint64_t n_items,
                      int add_omit, uint32_t R, const uint8_t* d_omit, const uint64_t* d_dst_off, uint8_t* d_out, const OnlineList* d_ol, uint32_t rep_min) {
    if (!n_items) return;
    if (d_ol) {
        const uint64_t threads = n_items * RV_ONLINE_REPS;
        launch<B_k_extract64_ol, 256>(k_extract64_ol, st, dim3((unsigned)((threads + 255) / 256)), dim3(256), d_stream, stride_words, d_offs,
                                      n_items, add_omit, d_ol, d_omit, d_dst_off, d_out, rep_min);
        return;
    }
    const uint64_t threads = n_items * R;
    launch<B_k_extract64, 256>(k_extract64, st, dim3((unsigned)((threads + 255) / 256)), dim3(256), d_stream, stride_words, d_offs,
                               n_items, add_omit, R, d_omit, d_dst_off, d_out);
}

// verifier: proof vectors -> dense [item][out_r] u64 (out_r = R, or the first 64 repetitions when no other is opened -- the
// verifier's slot order: a quarter of the bytes); items past a vector's end read as zero
// (z64/recon.rs:96-104, z64/share.rs:78-88 `unwrap_or([0u8; 8])`)
struct B_k_unpack64 {
    __device__ __forceinline__ void operator()(const uint8_t* __restrict__ blob, const uint64_t* __restrict__ src_off,
                                               const uint64_t* __restrict__ src_len, const uint8_t* __restrict__ omit, uint64_t n_items, uint32_t out_r,
                                               uint64_t* __restrict__ out) const {
#include "z64_unpack.inc"
}
};
__global__ void k_unpack64(const uint8_t* __restrict__ blob, const uint64_t* __restrict__ src_off,
                           const uint64_t* __restrict__ src_len, const uint8_t* __restrict__ omit, uint64_t n_items, uint32_t out_r,
                           uint64_t* __restrict__ out) {
#include "z64_unpack.inc"
}

void launch_unpack64(hipStream_t st, const uint8_t* d_blob, const uint64_t* d_src_off, const uint64_t* d_src_len,
                     const uint8_t* d_omit, uint64_t n_items, uint32_t R, uint64_t* d_out, uint32_t out_r) {
    if (!n_items) return;
    (void)R;
    const uint64_t threads = n_items * out_r;
    launch<B_k_unpack64, 256>(k_unpack64, st, dim3((unsigned)((threads + 255) / 256)), dim3(256), d_blob, d_src_off, d_src_len, d_omit,
                              n_items, out_r, d_out);
}

}  // namespace rv
