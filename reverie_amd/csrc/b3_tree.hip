// BLAKE3 transcript trees for gfx950: chunk kernels over the row-format transcripts, the tree reductions, the incremental
// tree of the streaming prover and the digest joins.  (The interpreter that writes the transcripts: interp.hip.)
//
// Replaces (all under the reference's src/):
//   crypto/hash.rs:17-104             BufferedHasher / PackedHasher (per-rep BLAKE3 streams)
//   transcript/mod.rs:77-96, interpreter/combine.rs:104-118   digest joins
#include <algorithm>

#include "b3.h"
#include "internal.h"
#include "launch.h"

namespace rv {

#ifndef RV_B3_RPL
#define RV_B3_RPL 4
#endif

// ------------------------------------------------------------------------------------
// BLAKE3 over row-format transcripts.  Thread = (chunk, quad): reads 64 rows per block
// (coalesced across the quads of a row), de-interleaves the 4 repetitions of its quad
// word into 4 x 16 message words and runs the 4 compressions back to back.
// ------------------------------------------------------------------------------------
// RPL = repetitions per lane (4: one lane per quad word; 1: four lanes share a quad word).  Fewer
// repetitions per lane = more, lighter wavefronts: 4 900 chunks x 64 lanes is only 1.6 rounds of the
// chip at 3 waves/SIMD (40 % of the time is tail), RPL = 1 gives 19 600 waves at 7+ waves/SIMD.
// UNI (RPL = 4, full-width rows, no quad list: the prover's whole proofs): a chunk per wavefront, lane = quad word.  The chunk index
// is then wave-uniform BY CONSTRUCTION, so a block's 64 row loads take a scalar base and one shared 32-bit lane offset instead of
// 64 vector address computations (128 of ~3 200 VALU instructions per block).
template <int RPL, bool UNI = false>
struct B_k_b3_chunks {
    // quads (nullable) / n_quads: only these quad words are hashed -- the verifier needs the online digest of the 40
    // opened repetitions alone (the other 216 carry theirs in the proof), i.e. of at most 40 of the 64 quads
    // chunk_base / root_ok (streaming prover): the stream handed in is a piece of a longer one -- its first chunk has
    // BLAKE3 chunk counter chunk_base, and a lone chunk only takes the ROOT flag when the caller knows it is the whole stream
    __device__ __forceinline__ void operator()(const uint32_t* __restrict__ stream, uint64_t n_events, uint32_t NQ, uint64_t n_chunks, uint32_t* __restrict__ cvs /*[n_chunks][R][8]*/, const uint32_t* __restrict__ quads, uint32_t n_quads, uint64_t chunk_base, uint32_t root_ok) const {
    run((uint64_t)blockIdx.x * blockDim.x + threadIdx.x, stream, n_events, NQ, n_chunks, cvs, quads, n_quads, chunk_base, root_ok);
    }
    static __device__ __forceinline__ void run(uint64_t tid, const uint32_t* __restrict__ stream, uint64_t n_events, uint32_t NQ, uint64_t n_chunks, uint32_t* __restrict__ cvs, const uint32_t* __restrict__ quads, uint32_t n_quads, uint64_t chunk_base, uint32_t root_ok) {
    constexpr uint32_t SUBS = 4 / RPL;
    static_assert(!UNI || RPL == 4, "a chunk per wavefront needs one lane per quad word");
    const uint32_t lanes_per_chunk = UNI ? 64u : (quads ? n_quads : NQ) * SUBS;
    uint64_t c = tid / lanes_per_chunk;
    if (UNI) c = (uint64_t)__builtin_amdgcn_readfirstlane((uint32_t)c) | ((uint64_t)__builtin_amdgcn_readfirstlane((uint32_t)(c >> 32)) << 32);
    const uint32_t ql = (uint32_t)(tid % lanes_per_chunk);
    const uint32_t q = UNI ? ql : (quads ? quads[ql / SUBS] : ql / SUBS), sub = ql % SUBS;
    if (c >= n_chunks) return;
    const uint64_t ev0 = c * 1024;
    const uint64_t len = (n_events - ev0 < 1024) ? (n_events - ev0) : 1024;
    const uint32_t nblk = len == 0 ? 1 : (uint32_t)((len + 63) / 64);
    uint32_t cv[RPL][8];
#pragma unroll
    for (int i = 0; i < RPL; i++) b3::iv(cv[i]);
    for (uint32_t b = 0; b < nblk; b++) {
        const uint64_t e0 = ev0 + 64ull * b;
        const uint32_t blen = (b + 1 < nblk) ? 64u : (uint32_t)(len - 64ull * b);
        uint32_t flags = (b == 0 ? b3::CHUNK_START : 0u) | (b + 1 == nblk ? b3::CHUNK_END : 0u);
        if (b + 1 == nblk && n_chunks == 1 && root_ok) flags |= b3::ROOT;
        uint32_t w[64];
        if (blen == 64) {
            // unguarded: a per-element "load or zero" select makes hipcc branch around every load and
            // wait for it (64 dependent round trips per block)
            if (UNI) {
                const char* rb = (const char*)(stream + e0 * 64);
                const uint32_t qoff = q * 4u;
#pragma unroll
                for (int e = 0; e < 64; e++) w[e] = *(const uint32_t*)(rb + e * 256 + qoff);
            } else {
#pragma unroll
                for (int e = 0; e < 64; e++) w[e] = stream[(e0 + e) * NQ + q];
            }
        } else {
#pragma unroll
            for (int e = 0; e < 64; e++) w[e] = (e0 + e < n_events) ? stream[(e0 + e) * NQ + q] : 0u;
        }
        uint32_t m[RPL][16];
#pragma unroll
        for (int i = 0; i < RPL; i++) {
            const uint32_t i4 = sub * RPL + i;  // repetition inside the quad word; its byte counts from the MSB
            const uint32_t sel = 3 - i4;        // byte index for v_perm (0 = LSB)
#pragma unroll
            for (int k = 0; k < 16; k++) {
                // m = byte(w[4k]) | byte(w[4k+1]) << 8 | byte(w[4k+2]) << 16 | byte(w[4k+3]) << 24: two v_perm_b32
                const uint32_t lo = __builtin_amdgcn_perm(w[4 * k + 1], w[4 * k], 0x0c0c0400u + sel * 0x0101u);
                const uint32_t hi = __builtin_amdgcn_perm(w[4 * k + 3], w[4 * k + 2], 0x0c0c0400u + sel * 0x0101u);
                m[i][k] = lo | (hi << 16);
            }
        }
        b3::compress_n<RPL>(cv, m, c + chunk_base, blen, flags);  // the lane's repetitions in lockstep
    }
    const uint32_t R = NQ * 4;
#pragma unroll
    for (int i = 0; i < RPL; i++) {
        uint32_t* dst = cvs + ((size_t)c * R + 4 * q + sub * RPL + i) * 8;
#pragma unroll
        for (int k = 0; k < 8; k++) dst[k] = cv[i][k];
    }
}
};
template <int RPL>
__global__ __launch_bounds__(256) void k_b3_chunks(const uint32_t* __restrict__ stream, uint64_t n_events, uint32_t NQ, uint64_t n_chunks, uint32_t* __restrict__ cvs /*[n_chunks][R][8]*/, const uint32_t* __restrict__ quads, uint32_t n_quads, uint64_t chunk_base, uint32_t root_ok) {
    B_k_b3_chunks<RPL>{}(stream, n_events, NQ, n_chunks, cvs, quads, n_quads, chunk_base, root_ok);
}
__global__ __launch_bounds__(256) void k_b3_chunks_uni(const uint32_t* __restrict__ stream, uint64_t n_events, uint32_t NQ, uint64_t n_chunks, uint32_t* __restrict__ cvs /*[n_chunks][R][8]*/, const uint32_t* __restrict__ quads, uint32_t n_quads, uint64_t chunk_base, uint32_t root_ok) {
    B_k_b3_chunks<4, true>{}(stream, n_events, NQ, n_chunks, cvs, quads, n_quads, chunk_base, root_ok);
}

// Same for a bit-per-rep transcript (the preprocessing stream): every bit is hashed as the
// 0x00/0xFF byte the reference feeds its hasher (gf2/recon.rs:314-321).
// RPL as in k_b3_chunks: 4 = one lane per quad word, 1 = four lanes share it (short transcripts: more, lighter wavefronts)
template <int RPL, bool UNI = false>
struct B_k_b3_chunks_bits {
    __device__ __forceinline__ void operator()(const uint8_t* __restrict__ stream, uint64_t n_events, uint32_t NQ, uint64_t n_chunks, uint32_t* __restrict__ cvs, uint64_t chunk_base, uint32_t root_ok) const {
    run((uint64_t)blockIdx.x * blockDim.x + threadIdx.x, stream, n_events, NQ, n_chunks, cvs, chunk_base, root_ok);
    }
    static __device__ __forceinline__ void run(uint64_t tid, const uint8_t* __restrict__ stream, uint64_t n_events, uint32_t NQ, uint64_t n_chunks, uint32_t* __restrict__ cvs, uint64_t chunk_base, uint32_t root_ok) {
    constexpr uint32_t SUBS = 4 / RPL;
    static_assert(!UNI || RPL == 4, "a chunk per wavefront needs one lane per quad word");
    const uint32_t lanes_per_chunk = UNI ? 64u : NQ * SUBS;  // (UNI: NQ = 64, see B_k_b3_chunks)
    uint64_t c = tid / lanes_per_chunk;
    if (UNI) c = (uint64_t)__builtin_amdgcn_readfirstlane((uint32_t)c) | ((uint64_t)__builtin_amdgcn_readfirstlane((uint32_t)(c >> 32)) << 32);
    const uint32_t ql = (uint32_t)(tid % lanes_per_chunk);
    const uint32_t q = ql / SUBS, sub = ql % SUBS;
    if (c >= n_chunks) return;
    const uint64_t ev0 = c * 1024;
    const uint64_t len = (n_events - ev0 < 1024) ? (n_events - ev0) : 1024;
    const uint32_t nblk = len == 0 ? 1 : (uint32_t)((len + 63) / 64);
    const uint32_t h = NQ >> 1, o = q >> 1, sh = 4 * (q & 1);
    uint32_t cv[RPL][8];
#pragma unroll
    for (int i = 0; i < RPL; i++) b3::iv(cv[i]);
    for (uint32_t b = 0; b < nblk; b++) {
        const uint64_t e0 = ev0 + 64ull * b;
        const uint32_t blen = (b + 1 < nblk) ? 64u : (uint32_t)(len - 64ull * b);
        uint32_t flags = (b == 0 ? b3::CHUNK_START : 0u) | (b + 1 == nblk ? b3::CHUNK_END : 0u);
        if (b + 1 == nblk && n_chunks == 1 && root_ok) flags |= b3::ROOT;
        // P = the nibbles of events 4k..4k+3, one per byte; repetition i4 owns nibble bit 3-i4
        uint32_t m[RPL][16];
        uint32_t nbs[64];
        if (blen == 64) {
            if (UNI) {
                const uint8_t* rb = stream + e0 * 32;
#pragma unroll
                for (int e = 0; e < 64; e++) nbs[e] = *(rb + e * 32 + o);
            } else {
#pragma unroll
                for (int e = 0; e < 64; e++) nbs[e] = stream[(e0 + e) * h + o];
            }
        } else {
#pragma unroll
            for (int e = 0; e < 64; e++) nbs[e] = (e0 + e < n_events) ? (uint32_t)stream[(e0 + e) * h + o] : 0u;
        }
#pragma unroll
        for (int k = 0; k < 16; k++) {
            uint32_t P = 0;
#pragma unroll
            for (int j = 0; j < 4; j++) P |= ((nbs[4 * k + j] >> sh) & 0xFu) << (8 * j);
#pragma unroll
            for (int i = 0; i < RPL; i++) {
                const uint32_t i4 = sub * RPL + i;
                const uint32_t t = (P >> (3 - i4)) & 0x01010101u;
                m[i][k] = (t << 8) - t;
            }
        }
        b3::compress_n<RPL>(cv, m, c + chunk_base, blen, flags);
    }
    const uint32_t R = NQ * 4;
#pragma unroll
    for (int i = 0; i < RPL; i++) {
        uint32_t* dst = cvs + ((size_t)c * R + 4 * q + sub * RPL + i) * 8;
#pragma unroll
        for (int k = 0; k < 8; k++) dst[k] = cv[i][k];
    }
}
};
__global__ __launch_bounds__(256) void k_b3_chunks_bits(const uint8_t* __restrict__ stream, uint64_t n_events, uint32_t NQ, uint64_t n_chunks, uint32_t* __restrict__ cvs, uint64_t chunk_base, uint32_t root_ok) {
    B_k_b3_chunks_bits<4>{}(stream, n_events, NQ, n_chunks, cvs, chunk_base, root_ok);
}
__global__ __launch_bounds__(256) void k_b3_chunks_bits_uni(const uint8_t* __restrict__ stream, uint64_t n_events, uint32_t NQ, uint64_t n_chunks, uint32_t* __restrict__ cvs, uint64_t chunk_base, uint32_t root_ok) {
    B_k_b3_chunks_bits<4, true>{}(stream, n_events, NQ, n_chunks, cvs, chunk_base, root_ok);
}
__global__ __launch_bounds__(256) void k_b3_chunks_bits1(const uint8_t* __restrict__ stream, uint64_t n_events, uint32_t NQ, uint64_t n_chunks, uint32_t* __restrict__ cvs, uint64_t chunk_base, uint32_t root_ok) {
    B_k_b3_chunks_bits<1>{}(stream, n_events, NQ, n_chunks, cvs, chunk_base, root_ok);
}

// LG tree levels per launch: thread = (group of G = 2^LG consecutive nodes, repetition).  One level is
// out[i] = parent(in[2i], in[2i+1]) with an odd last node promoted unchanged; groups are aligned to G, so
// reducing a group locally level by level gives exactly the nodes LG global levels would (the ragged
// last group follows the same promote rule).  The ROOT flag belongs to the merge of the last two nodes of
// the whole tree, which can only happen inside the only group of a launch.
template <int LG>
struct B_k_b3_reduce {
    __device__ __forceinline__ void operator()(const uint32_t* __restrict__ in, uint64_t n_in, uint32_t R, uint32_t* __restrict__ out) const {
    run((uint64_t)blockIdx.x * blockDim.x + threadIdx.x, in, n_in, R, out);
    }
    static __device__ __forceinline__ void run(uint64_t tid, const uint32_t* __restrict__ in, uint64_t n_in, uint32_t R, uint32_t* __restrict__ out) {
    constexpr int G = 1 << LG;
    const uint64_t n_out = (n_in + G - 1) / G;
    const uint64_t g = tid / R;
    const uint32_t r = (uint32_t)(tid % R);
    if (g >= n_out) return;
    uint32_t cnt = (uint32_t)((n_in - G * g < (uint64_t)G) ? n_in - G * g : G);
    uint32_t cv[G][8];
#pragma unroll
    for (int i = 0; i < G; i++) {
        if ((uint32_t)i < cnt) {
            const uint4* src = (const uint4*)(in + ((size_t)(G * g + i) * R + r) * 8);
            const uint4 lo = src[0], hi = src[1];
            cv[i][0] = lo.x; cv[i][1] = lo.y; cv[i][2] = lo.z; cv[i][3] = lo.w;
            cv[i][4] = hi.x; cv[i][5] = hi.y; cv[i][6] = hi.z; cv[i][7] = hi.w;
        } else {
#pragma unroll
            for (int k = 0; k < 8; k++) cv[i][k] = 0;
        }
    }
#pragma unroll
    for (int lvl = 0; lvl < LG; lvl++) {
        const uint32_t flags = (n_out == 1 && cnt == 2) ? b3::ROOT : 0u;
#pragma unroll
        for (int i = 0; i < (G >> (lvl + 1)); i++) {
            if ((uint32_t)(2 * i + 1) < cnt) {
                uint32_t o[8];
                b3::parent(cv[2 * i], cv[2 * i + 1], flags, o);
#pragma unroll
                for (int k = 0; k < 8; k++) cv[i][k] = o[k];
            } else if ((uint32_t)(2 * i) < cnt) {
#pragma unroll
                for (int k = 0; k < 8; k++) cv[i][k] = cv[2 * i][k];
            }
        }
        cnt = (cnt + 1) / 2;
    }
    uint4* d = (uint4*)(out + ((size_t)g * R + r) * 8);
    d[0] = make_uint4(cv[0][0], cv[0][1], cv[0][2], cv[0][3]);
    d[1] = make_uint4(cv[0][4], cv[0][5], cv[0][6], cv[0][7]);
}
};
template <int LG>
__global__ __launch_bounds__(256) void k_b3_reduce(const uint32_t* __restrict__ in, uint64_t n_in, uint32_t R, uint32_t* __restrict__ out) {
    B_k_b3_reduce<LG>{}(in, n_in, R, out);
}

// The top of the tree (at most B3_TAIL nodes per repetition): one workgroup per repetition walks the
// remaining levels through LDS, a barrier per level instead of a launch per level.
constexpr uint32_t B3_TAIL = 512;
// CAP = most nodes the workgroup takes (its LDS footprint): B3_TAIL with 256 threads, or 64 with one wavefront for the
// short transcripts of small circuits -- 2.3 KB instead of 18 KB of LDS, so a batch of proofs gets four times the
// workgroups per CU
template <int CAP>
struct B_k_b3_tree_tail {
    __device__ __forceinline__ void operator()(const uint32_t* __restrict__ in, uint32_t n_in, uint32_t R, uint32_t* __restrict__ digest) const {
    run(blockIdx.x, in, n_in, R, digest);
    }
    static __device__ __forceinline__ void run(uint32_t r, const uint32_t* __restrict__ in, uint32_t n_in, uint32_t R, uint32_t* __restrict__ digest) {
    __shared__ uint32_t cv[CAP][8 + 1];  // +1: odd row stride, no bank conflicts on the strided pair reads
    for (uint32_t i = threadIdx.x; i < n_in * 8; i += blockDim.x) cv[i >> 3][i & 7] = in[((size_t)(i >> 3) * R + r) * 8 + (i & 7)];
    __syncthreads();
    uint32_t cnt = n_in;
    while (cnt > 1) {
        const uint32_t half = (cnt + 1) / 2;
        const uint32_t i = threadIdx.x;
        uint32_t o[8];
        if (i < half) {
            if (2 * i + 1 < cnt) {
                uint32_t l[8], rr[8];
#pragma unroll
                for (int k = 0; k < 8; k++) {
                    l[k] = cv[2 * i][k];
                    rr[k] = cv[2 * i + 1][k];
                }
                b3::parent(l, rr, cnt == 2 ? b3::ROOT : 0u, o);
            } else {
#pragma unroll
                for (int k = 0; k < 8; k++) o[k] = cv[2 * i][k];
            }
        }
        __syncthreads();
        if (i < half) {
#pragma unroll
            for (int k = 0; k < 8; k++) cv[i][k] = o[k];
        }
        __syncthreads();
        cnt = half;
    }
    if (threadIdx.x < 8) digest[(size_t)r * 8 + threadIdx.x] = cv[0][threadIdx.x];
}
};
__global__ __launch_bounds__(256) void k_b3_tree_tail(const uint32_t* __restrict__ in, uint32_t n_in, uint32_t R, uint32_t* __restrict__ digest) {
    B_k_b3_tree_tail<(int)B3_TAIL>{}(in, n_in, R, digest);
}
__global__ __launch_bounds__(64) void k_b3_tree_tail_small(const uint32_t* __restrict__ in, uint32_t n_in, uint32_t R, uint32_t* __restrict__ digest) {
    B_k_b3_tree_tail<64>{}(in, n_in, R, digest);
}

// The same top of the tree with ONE LANE per repetition (at most 64 chaining values): the lane folds its values the way
// the incremental hasher does -- complete subtrees of 2^k chunks wait in slot k, the last value closes them from the
// smallest up and the last parent carries ROOT -- n - 1 dependent compressions, but 64 repetitions per wavefront instead
// of one.  For a batch of proofs that is the difference between 65 536 workgroups of one mostly idle wavefront each
// (rv_prove_batch of 256 AES-128 proofs: 2 x 261 us) and 1 024 full wavefronts.
struct B_k_b3_tree_lane {
    __device__ __forceinline__ void operator()(const uint32_t* __restrict__ in, uint32_t n_in, uint32_t R, uint32_t* __restrict__ digest) const {
    const uint32_t r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= R) return;
    auto load = [&](uint32_t i, uint32_t* cv) {
        const uint4* p = (const uint4*)(in + ((size_t)i * R + r) * 8);
        const uint4 a = p[0], b = p[1];
        cv[0] = a.x, cv[1] = a.y, cv[2] = a.z, cv[3] = a.w, cv[4] = b.x, cv[5] = b.y, cv[6] = b.z, cv[7] = b.w;
    };
    uint32_t st[6][8], cur[8], o[8];
    for (uint32_t i = 0; i + 1 < n_in; i++) {  // (uniform: every lane walks the same tree shape)
        load(i, cur);
        bool placed = false;
#pragma unroll
        for (int k = 0; k < 6; k++) {
            if (placed) continue;
            if ((i >> k) & 1u) {
                b3::parent(st[k], cur, 0u, o);
#pragma unroll
                for (int w = 0; w < 8; w++) cur[w] = o[w];
            } else {
#pragma unroll
                for (int w = 0; w < 8; w++) st[k][w] = cur[w];
                placed = true;
            }
        }
    }
    const uint32_t last = n_in - 1;
    load(last, cur);  // a single chunk is already its own root (the chunk kernels applied the ROOT flag)
#pragma unroll
    for (int k = 0; k < 6; k++) {
        if ((last >> k) & 1u) {
            b3::parent(st[k], cur, (last >> (k + 1)) == 0 ? b3::ROOT : 0u, o);
#pragma unroll
            for (int w = 0; w < 8; w++) cur[w] = o[w];
        }
    }
    uint4* d = (uint4*)(digest + (size_t)r * 8);
    d[0] = make_uint4(cur[0], cur[1], cur[2], cur[3]);
    d[1] = make_uint4(cur[4], cur[5], cur[6], cur[7]);
}
};
__global__ __launch_bounds__(64) void k_b3_tree_lane(const uint32_t* __restrict__ in, uint32_t n_in, uint32_t R, uint32_t* __restrict__ digest) {
    B_k_b3_tree_lane{}(in, n_in, R, digest);
}

// Both transcripts of a small proof in the same two launches.  With a handful of chunks per stream the chunk kernels are
// one dependent chain of 16 compressions per lane (~37 us) whatever the number of lanes, and the tree tops a few more:
// run back to back, preprocessing then online, they are ~90 us of a 0.55 ms AES-128 proof.  The first blocks of a paired
// launch take the preprocessing stream, the rest the online one (one repetition per lane in both).
struct B_k_b3_chunks_pair {
    __device__ __forceinline__ void operator()(const uint8_t* __restrict__ pre, uint64_t n_pre, uint32_t* __restrict__ cv_pre, const uint32_t* __restrict__ on,
                                               uint64_t n_on, uint32_t* __restrict__ cv_on, uint32_t NQ, uint32_t blocks_pre, const uint32_t* __restrict__ quads,
                                               uint32_t n_quads) const {
    const uint64_t c_pre = n_pre == 0 ? 1 : (n_pre + 1023) / 1024, c_on = n_on == 0 ? 1 : (n_on + 1023) / 1024;
    if (blockIdx.x < blocks_pre)
        B_k_b3_chunks_bits<1>::run((uint64_t)blockIdx.x * blockDim.x + threadIdx.x, pre, n_pre, NQ, c_pre, cv_pre, 0, 1);
    else
        B_k_b3_chunks<1>::run((uint64_t)(blockIdx.x - blocks_pre) * blockDim.x + threadIdx.x, on, n_on, NQ, c_on, cv_on, quads, n_quads, 0, 1);
    }
};
__global__ __launch_bounds__(256) void k_b3_chunks_pair(const uint8_t* __restrict__ pre, uint64_t n_pre, uint32_t* __restrict__ cv_pre, const uint32_t* __restrict__ on,
                                                        uint64_t n_on, uint32_t* __restrict__ cv_on, uint32_t NQ, uint32_t blocks_pre,
                                                        const uint32_t* __restrict__ quads, uint32_t n_quads) {
    B_k_b3_chunks_pair{}(pre, n_pre, cv_pre, on, n_on, cv_on, NQ, blocks_pre, quads, n_quads);
}
// ONE small proof (no batch to supply wavefronts): a chunk's 16 chained compressions are the whole duration of the chunk launch, so
// each repetition's chain runs on a QUAD of lanes (b3.h: compress_q) -- lane = (chunk, repetition, column).  A lane assembles the four
// message words of its column's share of the block (16 of the block's 64 rows), the quad exchanges them through LDS.  ~37 -> ~15 us.
// BITS: the preprocessing stream (a bit per repetition and event); else the online stream (a byte).  quads / n_quads as in
// B_k_b3_chunks; a quad of lanes never straddles two chunks, so its four lanes always run the same number of blocks.
template <bool BITS>
struct B_k_b3_chunks_q {
    static __device__ __forceinline__ void run(uint64_t tid, const void* __restrict__ stream, uint64_t n_events, uint32_t NQ, uint64_t n_chunks, uint32_t* __restrict__ cvs,
                                               const uint32_t* __restrict__ quads, uint32_t n_quads, uint32_t* s_msg /* [threads / 4][16] */) {
    const uint32_t qc = (uint32_t)(tid & 3);
    const uint32_t reps_per_chunk = (quads ? n_quads : NQ) * 4;
    const uint64_t gi = tid >> 2;  // (chunk, repetition slot)
    const uint64_t c = gi / reps_per_chunk;
    const uint32_t rs = (uint32_t)(gi % reps_per_chunk);
    if (c >= n_chunks) return;  // (whole quads leave together)
    const uint32_t q = quads ? quads[rs >> 2] : rs >> 2, i4 = rs & 3;
    uint32_t* const msg = s_msg + (threadIdx.x >> 2) * 16;
    const b3::QuadSchedule qs = b3::quad_schedule(qc);
    const uint64_t ev0 = c * 1024;
    const uint64_t len = (n_events - ev0 < 1024) ? (n_events - ev0) : 1024;
    const uint32_t nblk = len == 0 ? 1 : (uint32_t)((len + 63) / 64);
    uint32_t cva = qc == 0 ? B3_IV0 : qc == 1 ? B3_IV1 : qc == 2 ? B3_IV2 : B3_IV3;
    uint32_t cvb = qc == 0 ? B3_IV4 : qc == 1 ? B3_IV5 : qc == 2 ? B3_IV6 : B3_IV7;
    // this lane's 16 rows of block b (message words 4 qc .. 4 qc + 3), one word each (a byte of the bit rows); the rows of block b + 1
    // are requested before block b is compressed -- a memory round trip per block was most of the chain
    const uint32_t h = NQ >> 1, o = q >> 1, sh = 4 * (q & 1);
    auto load_rows = [&](uint32_t b, uint32_t (&w)[16]) {
        const uint64_t e0 = ev0 + 64ull * b + 16ull * qc;
#pragma unroll
        for (int e = 0; e < 16; e++) {
            if (BITS)
                w[e] = (e0 + e < n_events) ? (uint32_t)((const uint8_t*)stream)[(e0 + e) * h + o] : 0u;
            else
                w[e] = (e0 + e < n_events) ? ((const uint32_t*)stream)[(e0 + e) * NQ + q] : 0u;
        }
    };
    uint32_t w[16];
    load_rows(0, w);
    for (uint32_t b = 0; b < nblk; b++) {
        const uint32_t blen = (b + 1 < nblk) ? 64u : (uint32_t)(len - 64ull * b);
        uint32_t flags = (b == 0 ? b3::CHUNK_START : 0u) | (b + 1 == nblk ? b3::CHUNK_END : 0u);
        if (b + 1 == nblk && n_chunks == 1) flags |= b3::ROOT;
        uint32_t m4[4];
        if (BITS) {
#pragma unroll
            for (int kk = 0; kk < 4; kk++) {
                uint32_t P = 0;
#pragma unroll
                for (int j = 0; j < 4; j++) P |= ((w[4 * kk + j] >> sh) & 0xFu) << (8 * j);
                const uint32_t t = (P >> (3 - i4)) & 0x01010101u;
                m4[kk] = (t << 8) - t;
            }
        } else {
            const uint32_t sel = 3 - i4;  // byte index for v_perm (0 = LSB): the repetition's byte counts from the MSB
#pragma unroll
            for (int kk = 0; kk < 4; kk++) {
                const uint32_t lo = __builtin_amdgcn_perm(w[4 * kk + 1], w[4 * kk], 0x0c0c0400u + sel * 0x0101u);
                const uint32_t hi = __builtin_amdgcn_perm(w[4 * kk + 3], w[4 * kk + 2], 0x0c0c0400u + sel * 0x0101u);
                m4[kk] = lo | (hi << 16);
            }
        }
        if (b + 1 < nblk) load_rows(b + 1, w);
        // (the quad's lanes sit in one wavefront, whose LDS accesses execute in order: the block's reads of the step before are done)
#pragma unroll
        for (int kk = 0; kk < 4; kk++) msg[4 * qc + kk] = m4[kk];
        __builtin_amdgcn_wave_barrier();
        b3::compress_q<false>(cva, cvb, msg, qs, qc, c, blen, flags);
        __builtin_amdgcn_wave_barrier();
    }
    const uint32_t R = NQ * 4;
    uint32_t* dst = cvs + ((size_t)c * R + 4 * q + i4) * 8;
    dst[qc] = cva;
    dst[4 + qc] = cvb;
    }
};
struct B_k_b3_chunks_pair_q {
    __device__ __forceinline__ void operator()(const uint8_t* __restrict__ pre, uint64_t n_pre, uint32_t* __restrict__ cv_pre, const uint32_t* __restrict__ on,
                                               uint64_t n_on, uint32_t* __restrict__ cv_on, uint32_t NQ, uint32_t blocks_pre, const uint32_t* __restrict__ quads,
                                               uint32_t n_quads) const {
    __shared__ uint32_t s_msg[64 * 16];
    const uint64_t c_pre = n_pre == 0 ? 1 : (n_pre + 1023) / 1024, c_on = n_on == 0 ? 1 : (n_on + 1023) / 1024;
    if (blockIdx.x < blocks_pre)
        B_k_b3_chunks_q<true>::run((uint64_t)blockIdx.x * blockDim.x + threadIdx.x, pre, n_pre, NQ, c_pre, cv_pre, nullptr, 0, s_msg);
    else
        B_k_b3_chunks_q<false>::run((uint64_t)(blockIdx.x - blocks_pre) * blockDim.x + threadIdx.x, on, n_on, NQ, c_on, cv_on, quads, n_quads, s_msg);
    }
};
__global__ __launch_bounds__(256) void k_b3_chunks_pair_q(const uint8_t* __restrict__ pre, uint64_t n_pre, uint32_t* __restrict__ cv_pre, const uint32_t* __restrict__ on,
                                                          uint64_t n_on, uint32_t* __restrict__ cv_on, uint32_t NQ, uint32_t blocks_pre,
                                                          const uint32_t* __restrict__ quads, uint32_t n_quads) {
    B_k_b3_chunks_pair_q{}(pre, n_pre, cv_pre, on, n_on, cv_on, NQ, blocks_pre, quads, n_quads);
}
// tree tops of both: workgroups [0, R) the preprocessing stream, [R, 2R) the online one
struct B_k_b3_tree_tail_pair {
    __device__ __forceinline__ void operator()(const uint32_t* __restrict__ in_a, uint32_t n_a, uint32_t* __restrict__ dig_a, const uint32_t* __restrict__ in_b, uint32_t n_b,
                                               uint32_t* __restrict__ dig_b, uint32_t R) const {
    if (blockIdx.x < R)
        B_k_b3_tree_tail<64>::run(blockIdx.x, in_a, n_a, R, dig_a);
    else
        B_k_b3_tree_tail<64>::run(blockIdx.x - R, in_b, n_b, R, dig_b);
    }
};
__global__ __launch_bounds__(64) void k_b3_tree_tail_pair(const uint32_t* __restrict__ in_a, uint32_t n_a, uint32_t* __restrict__ dig_a, const uint32_t* __restrict__ in_b,
                                                          uint32_t n_b, uint32_t* __restrict__ dig_b, uint32_t R) {
    B_k_b3_tree_tail_pair{}(in_a, n_a, dig_a, in_b, n_b, dig_b, R);
}
// The launchers below decide and launch in two steps: a b3_choose_* / b3_plan_* function says which kernel takes a shape (pure: the
// batch of the calling thread's recorder is an argument -- 0: no recorder), a launch_*_as / *_run function issues it.  Production calls
// the first and hands its answer to the second; the kernel tests (hooks_b3.inc: rv_hook_b3_*) call the second with any choice that takes the
// shape, so every kernel is reachable at small shapes, and tests/test_b3_plan_host.py pins the choices (rv_hook_b3_plan).
static inline uint32_t b3_batch_now() { return g_recorder ? std::max(g_recorder->batch, 1u) : 0u; }
static inline uint64_t b3_chunks_of(uint64_t n_events) { return n_events == 0 ? 1 : (n_events + 1023) / 1024; }

// are both streams short enough for the paired kernels, and in which form?  d_quads / n_quads as in launch_b3_stream (the verifier
// hashes the online stream of the opened quads only; n_quads = 0 with a list: not paired)
B3PairSmall b3_choose_pair_small(uint64_t n_pre, uint64_t n_on, uint32_t NQ, bool listed, uint32_t n_quads, uint32_t batch) {
    if (listed && !n_quads) return B3P_NONE;
    const uint64_t c_pre = b3_chunks_of(n_pre), c_on = b3_chunks_of(n_on);
    // (the same "few chunks" rule as the separate launchers' one-repetition-per-lane choice, and trees the small tail kernel takes)
    if (c_pre > 64 || c_on > 64 || std::max(c_pre, c_on) * NQ * (batch ? batch : 1u) >= 64 * 1024) return B3P_NONE;
    return batch ? B3P_LANE : B3P_QUAD;  // (one proof: a quad of lanes per repetition's chain)
}
// two launches; d_cv_a / d_cv_b each hold one stream's chunk chaining values (the tree tops need no second buffer at this size)
void launch_b3_pair_small_as(hipStream_t st, B3PairSmall form, const uint8_t* d_pre, uint64_t n_pre, const uint32_t* d_on, uint64_t n_on, uint32_t NQ,
                             uint32_t* d_cv_a, uint32_t* d_cv_b, uint32_t* d_dig_pre, uint32_t* d_dig_on, const uint32_t* d_quads, uint32_t n_quads) {
    const uint64_t c_pre = b3_chunks_of(n_pre), c_on = b3_chunks_of(n_on);
    const uint32_t R = NQ * 4;
    if (form == B3P_QUAD) {
        const uint32_t b_pre = (uint32_t)((c_pre * NQ * 16 + 255) / 256), b_on = (uint32_t)((c_on * (d_quads ? n_quads : NQ) * 16 + 255) / 256);
        hipLaunchKernelGGL(k_b3_chunks_pair_q, dim3(b_pre + b_on), dim3(256), 0, st, d_pre, n_pre, d_cv_a, d_on, n_on, d_cv_b, NQ, b_pre, d_quads, n_quads);
    } else {
    const uint32_t b_pre = (uint32_t)((c_pre * NQ * 4 + 255) / 256), b_on = (uint32_t)((c_on * (d_quads ? n_quads : NQ) * 4 + 255) / 256);
    launch<B_k_b3_chunks_pair, 256>(k_b3_chunks_pair, st, dim3(b_pre + b_on), dim3(256), d_pre, n_pre, d_cv_a, d_on, n_on, d_cv_b, NQ, b_pre, d_quads, n_quads);
    }
    launch<B_k_b3_tree_tail_pair, 64>(k_b3_tree_tail_pair, st, dim3(2 * R), dim3(64), (const uint32_t*)d_cv_a, (uint32_t)c_pre, d_dig_pre,
                                      (const uint32_t*)d_cv_b, (uint32_t)c_on, d_dig_on, R);
}
// true (and two launches issued) when both streams are short enough for the paired kernels
bool launch_b3_pair_small(hipStream_t st, const uint8_t* d_pre, uint64_t n_pre, const uint32_t* d_on, uint64_t n_on, uint32_t NQ, uint32_t* d_cv_a,
                          uint32_t* d_cv_b, uint32_t* d_dig_pre, uint32_t* d_dig_on, const uint32_t* d_quads, uint32_t n_quads) {
    const B3PairSmall form = b3_choose_pair_small(n_pre, n_on, NQ, d_quads != nullptr, n_quads, b3_batch_now());
    if (form == B3P_NONE) return false;
    launch_b3_pair_small_as(st, form, d_pre, n_pre, d_on, n_on, NQ, d_cv_a, d_cv_b, d_dig_pre, d_dig_on, d_quads, n_quads);
    return true;
}

// The trees of BOTH transcripts of a large proof in shared launches (blockIdx.y = the stream): after the two chunk kernels a whole
// proof of the 10^7-gate circuit ran two reduction launches and a tree top per stream, six dependent launches of ~20 us that each
// occupy a fraction of the chip -- three of them now.  A stream that is already at the tree top's size sits a reduction out.
// ... and their chunk kernels as ONE launch: the first workgroups hash the preprocessing stream (a bit per repetition), the others the online
// stream (a byte), a chunk per wavefront in both (B_k_b3_chunks<4, true>) -- the ragged last generation of the first fills with
// wavefronts of the second (on two streams that cost more in events than it gave: DESIGN.md section 4)
// (QUADS: the verifier -- the online stream of the quad words with an opened repetition only, a lane per listed quad word)
// (QUADS = 2: few listed quad words -- a quarter of the row or less --: a lane per REPETITION of them, as launch_b3_stream_chunks chooses)
template <int QUADS>
struct B_k_b3_chunks_pair_uni {
    __device__ __forceinline__ void operator()(const uint8_t* __restrict__ pre, uint64_t n_pre, uint32_t* __restrict__ cv_pre, const uint32_t* __restrict__ on,
                                               uint64_t n_on, uint32_t* __restrict__ cv_on, uint32_t blocks_pre, const uint32_t* __restrict__ quads, uint32_t n_quads) const {
    const uint64_t c_pre = n_pre == 0 ? 1 : (n_pre + 1023) / 1024, c_on = n_on == 0 ? 1 : (n_on + 1023) / 1024;
    if (blockIdx.x < blocks_pre)
        B_k_b3_chunks_bits<4, true>::run((uint64_t)blockIdx.x * blockDim.x + threadIdx.x, pre, n_pre, 64, c_pre, cv_pre, 0, 1);
    else if (QUADS == 2)
        B_k_b3_chunks<1, false>::run((uint64_t)(blockIdx.x - blocks_pre) * blockDim.x + threadIdx.x, on, n_on, 64, c_on, cv_on, quads, n_quads, 0, 1);
    else if (QUADS)
        B_k_b3_chunks<4, false>::run((uint64_t)(blockIdx.x - blocks_pre) * blockDim.x + threadIdx.x, on, n_on, 64, c_on, cv_on, quads, n_quads, 0, 1);
    else
        B_k_b3_chunks<4, true>::run((uint64_t)(blockIdx.x - blocks_pre) * blockDim.x + threadIdx.x, on, n_on, 64, c_on, cv_on, nullptr, 0, 0, 1);
    }
};
template <int QUADS>
__global__ __launch_bounds__(256) void k_b3_chunks_pair_uni(const uint8_t* __restrict__ pre, uint64_t n_pre, uint32_t* __restrict__ cv_pre, const uint32_t* __restrict__ on,
                                                            uint64_t n_on, uint32_t* __restrict__ cv_on, uint32_t blocks_pre, const uint32_t* __restrict__ quads,
                                                            uint32_t n_quads) {
    B_k_b3_chunks_pair_uni<QUADS>{}(pre, n_pre, cv_pre, on, n_on, cv_on, blocks_pre, quads, n_quads);
}
// (B3_TAIL_PAIR: the shared tree top takes up to 1 024 nodes per repetition with 512 threads, and a shared reduction launch folds THREE
// levels -- 4 900 chunks are 613 nodes after one launch, where two levels per launch and a 512-node top needed two launches)
constexpr uint32_t B3_TAIL_PAIR = 1024;
struct B_k_b3_reduce_pair {
    __device__ __forceinline__ void operator()(const uint32_t* __restrict__ in_a, uint64_t n_a, uint32_t* __restrict__ out_a, const uint32_t* __restrict__ in_b,
                                               uint64_t n_b, uint32_t* __restrict__ out_b, uint32_t R) const {
    const uint64_t tid = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (blockIdx.y == 0) {
        if (n_a > B3_TAIL_PAIR) B_k_b3_reduce<3>::run(tid, in_a, n_a, R, out_a);
    } else {
        if (n_b > B3_TAIL_PAIR) B_k_b3_reduce<3>::run(tid, in_b, n_b, R, out_b);
    }
    }
};
__global__ __launch_bounds__(256) void k_b3_reduce_pair(const uint32_t* __restrict__ in_a, uint64_t n_a, uint32_t* __restrict__ out_a, const uint32_t* __restrict__ in_b,
                                                        uint64_t n_b, uint32_t* __restrict__ out_b, uint32_t R) {
    B_k_b3_reduce_pair{}(in_a, n_a, out_a, in_b, n_b, out_b, R);
}
struct B_k_b3_tree_tail_pair_big {
    __device__ __forceinline__ void operator()(const uint32_t* __restrict__ in_a, uint32_t n_a, uint32_t* __restrict__ dig_a, const uint32_t* __restrict__ in_b, uint32_t n_b,
                                               uint32_t* __restrict__ dig_b, uint32_t R) const {
    if (blockIdx.x < R)
        B_k_b3_tree_tail<(int)B3_TAIL_PAIR>::run(blockIdx.x, in_a, n_a, R, dig_a);
    else
        B_k_b3_tree_tail<(int)B3_TAIL_PAIR>::run(blockIdx.x - R, in_b, n_b, R, dig_b);
    }
};
__global__ __launch_bounds__(512) void k_b3_tree_tail_pair_big(const uint32_t* __restrict__ in_a, uint32_t n_a, uint32_t* __restrict__ dig_a, const uint32_t* __restrict__ in_b,
                                                               uint32_t n_b, uint32_t* __restrict__ dig_b, uint32_t R) {
    B_k_b3_tree_tail_pair_big{}(in_a, n_a, dig_a, in_b, n_b, dig_b, R);
}
static uint64_t b3_rpl1_lanes();
// does launch_b3_pair_big take these two transcripts?  (both trees must end in the 256-thread tree top: more than 64 nodes left)
// recording: a recorder is present (a batch of proofs: never)
bool b3_pair_big_takes(uint64_t n_pre, uint64_t n_on, uint32_t NQ, bool listed_on, uint32_t n_quads, bool recording) {
    if (NQ != 64 || recording || RV_B3_RPL != 4) return false;
    if (listed_on && !n_quads) return false;
    for (int i = 0; i < 2; i++) {
        const uint64_t n_ev = i == 0 ? n_pre : n_on;
        const bool listed = i == 1 && listed_on;  // (the online stream of the listed quad words only)
        uint64_t n = b3_chunks_of(n_ev);
        // (short transcripts: the separate launchers pick other chunk kernels; few listed quad words are hashed a repetition per lane anyway)
        if (!(listed && n_quads * 4 <= NQ) && n * (listed ? std::min(n_quads, NQ) : NQ) < b3_rpl1_lanes()) return false;
        while (n > B3_TAIL_PAIR) n = (n + 7) / 8;
        if (n <= 64) return false;
    }
    return true;
}
bool b3_pair_big_ok(uint64_t n_pre, uint64_t n_on, uint32_t NQ, const uint32_t* d_quads, uint32_t n_quads) {
    return b3_pair_big_takes(n_pre, n_on, NQ, d_quads != nullptr, n_quads, g_recorder != nullptr);
}
// the shared reduction launches of two trees of n_a and n_b chaining values, and the nodes each has left for the shared tree top
B3PairBigPlan b3_plan_pair_big_tree(uint64_t n_a, uint64_t n_b) {
    B3PairBigPlan p{0, 0, 0};
    while (n_a > B3_TAIL_PAIR || n_b > B3_TAIL_PAIR) {
        if (n_a > B3_TAIL_PAIR) n_a = (n_a + 7) / 8;
        if (n_b > B3_TAIL_PAIR) n_b = (n_b + 7) / 8;
        p.reduces++;
    }
    p.top_a = (uint32_t)n_a, p.top_b = (uint32_t)n_b;
    return p;
}
// the chunk chaining values of both transcripts in one launch (NQ = 64): cv_a the preprocessing stream's, cv_b the online stream's
void launch_b3_pair_big_chunks(hipStream_t st, const uint8_t* d_pre, uint64_t n_pre, const uint32_t* d_on, uint64_t n_on, uint32_t* cv_a0, uint32_t* cv_b0,
                               const uint32_t* d_quads, uint32_t n_quads) {
    const uint32_t NQ = 64;
    const uint64_t n_a = b3_chunks_of(n_pre), n_b = b3_chunks_of(n_on);
    const uint32_t b_pre = (uint32_t)((n_a * 64 + 255) / 256);  // (a chunk per wavefront)
    if (d_quads && n_quads * 4 <= NQ) {
        // (the chaining values of skipped quad words stay whatever the buffer held: the tree above them runs on garbage and the caller
        // replaces those digests, as with launch_b3_stream)
        const uint32_t b_on = (uint32_t)((n_b * n_quads * 4 + 255) / 256);
        launch<B_k_b3_chunks_pair_uni<2>, 256>(k_b3_chunks_pair_uni<2>, st, dim3(b_pre + b_on), dim3(256), d_pre, n_pre, cv_a0, d_on, n_on, cv_b0, b_pre, d_quads,
                                              n_quads);
    } else if (d_quads) {
        const uint32_t b_on = (uint32_t)((n_b * n_quads + 255) / 256);
        launch<B_k_b3_chunks_pair_uni<1>, 256>(k_b3_chunks_pair_uni<1>, st, dim3(b_pre + b_on), dim3(256), d_pre, n_pre, cv_a0, d_on, n_on, cv_b0, b_pre, d_quads,
                                              n_quads);
    } else {
        const uint32_t b_on = (uint32_t)((n_b * 64 + 255) / 256);
        launch<B_k_b3_chunks_pair_uni<0>, 256>(k_b3_chunks_pair_uni<0>, st, dim3(b_pre + b_on), dim3(256), d_pre, n_pre, cv_a0, d_on, n_on, cv_b0, b_pre,
                                              (const uint32_t*)nullptr, 0u);
    }
}
// both trees over n_a / n_b chaining values in cv_a0 / cv_b0 (cv_a1 / cv_b1: the other halves of the ping-pong pairs) -> launches
uint32_t launch_b3_pair_big_tree(hipStream_t st, uint32_t* cv_a0, uint32_t* cv_a1, uint64_t n_a, uint32_t* cv_b0, uint32_t* cv_b1, uint64_t n_b, uint32_t R,
                                 uint32_t* d_dig_pre, uint32_t* d_dig_on) {
    uint32_t launches = 0;
    while (n_a > B3_TAIL_PAIR || n_b > B3_TAIL_PAIR) {
        const uint64_t out_a = (n_a + 7) / 8, out_b = (n_b + 7) / 8;
        const uint64_t threads = std::max(n_a > B3_TAIL_PAIR ? out_a : 0, n_b > B3_TAIL_PAIR ? out_b : 0) * R;
        launch<B_k_b3_reduce_pair, 256>(k_b3_reduce_pair, st, dim3((unsigned)((threads + 255) / 256), 2), dim3(256), (const uint32_t*)cv_a0, n_a, cv_a1,
                                        (const uint32_t*)cv_b0, n_b, cv_b1, R);
        if (n_a > B3_TAIL_PAIR) std::swap(cv_a0, cv_a1), n_a = out_a;
        if (n_b > B3_TAIL_PAIR) std::swap(cv_b0, cv_b1), n_b = out_b;
        launches++;
    }
    launch<B_k_b3_tree_tail_pair_big, 512>(k_b3_tree_tail_pair_big, st, dim3(2 * R), dim3(512), (const uint32_t*)cv_a0, (uint32_t)n_a, d_dig_pre,
                                           (const uint32_t*)cv_b0, (uint32_t)n_b, d_dig_on, R);
    return launches + 1;
}
// cv_a0 / cv_a1 and cv_b0 / cv_b1: ping-pong buffers of the preprocessing and the online stream (b3_stream_scratch_words each);
// -> launches
uint32_t launch_b3_pair_big(hipStream_t st, const uint8_t* d_pre, uint64_t n_pre, const uint32_t* d_on, uint64_t n_on, uint32_t NQ, uint32_t* cv_a0,
                            uint32_t* cv_a1, uint32_t* cv_b0, uint32_t* cv_b1, uint32_t* d_dig_pre, uint32_t* d_dig_on, const uint32_t* d_quads,
                            uint32_t n_quads) {
    launch_b3_pair_big_chunks(st, d_pre, n_pre, d_on, n_on, cv_a0, cv_b0, d_quads, n_quads);
    return 1 + launch_b3_pair_big_tree(st, cv_a0, cv_a1, b3_chunks_of(n_pre), cv_b0, cv_b1, b3_chunks_of(n_on), NQ * 4, d_dig_pre, d_dig_on);
}

// the launches of a tree over n chunk chaining values: k_b3_reduce<2> while the level is wider than the tree top takes, then the top.
// A single chunk is already its own root (the chunk kernels applied the ROOT flag): every top just copies it.
// Lane per repetition: always for a batch of proofs (gridDim.y supplies the parallelism), for a single proof only while
// its n - 1 dependent compressions (~1.2 us each) beat the workgroup version's log2(n) levels with their barriers
B3TreePlan b3_plan_tree(uint64_t n, uint32_t batch) {
    B3TreePlan p{0, 0, B3T_TAIL512};
    while (n > B3_TAIL) n = (n + 3) / 4, p.reduces++;  // two levels per launch while the level is wide
    p.n_top = (uint32_t)n;
    if (n <= 64 && (batch >= 8 || n <= 4))
        p.top = B3T_LANE;
    else if (n <= 64)
        p.top = B3T_TAIL64;
    return p;
}
// does this tree top take n nodes?  (k_b3_tree_lane: six slots; the workgroup tops: their LDS)
bool b3_top_takes(B3TopKernel top, uint64_t n) { return n >= 1 && n <= (top == B3T_TAIL512 ? B3_TAIL : 64u); }
// tree reduction of n chunk chaining values per repetition as planned; the roots land in d_digest ([R][8] words)
uint32_t b3_reduce_tree_run(hipStream_t st, const B3TreePlan& plan, uint32_t* cur, uint32_t* nxt, uint64_t n, uint32_t R, uint32_t* d_digest) {
    for (uint32_t i = 0; i < plan.reduces; i++) {
        const uint64_t n_out = (n + 3) / 4;
        const uint64_t threads = n_out * R;
        launch<B_k_b3_reduce<2>, 256>(k_b3_reduce<2>, st, dim3((unsigned)((threads + 255) / 256)), dim3(256), cur, n, R, nxt);
        uint32_t* t = cur;
        cur = nxt;
        nxt = t;
        n = n_out;
    }
    if (plan.top == B3T_LANE)
        launch<B_k_b3_tree_lane, 64>(k_b3_tree_lane, st, dim3((R + 63) / 64), dim3(64), cur, (uint32_t)n, R, d_digest);
    else if (plan.top == B3T_TAIL64)
        launch<B_k_b3_tree_tail<64>, 64>(k_b3_tree_tail_small, st, dim3(R), dim3(64), cur, (uint32_t)n, R, d_digest);
    else
        launch<B_k_b3_tree_tail<(int)B3_TAIL>, 256>(k_b3_tree_tail, st, dim3(R), dim3(256), cur, (uint32_t)n, R, d_digest);
    return plan.reduces + 1;
}
uint32_t b3_reduce_tree(hipStream_t st, uint32_t* cur, uint32_t* nxt, uint64_t n, uint32_t R, uint32_t* d_digest) {
    return b3_reduce_tree_run(st, b3_plan_tree(n, b3_batch_now()), cur, nxt, n, R, d_digest);
}

size_t b3_stream_scratch_words(uint64_t n_events, uint32_t R) {
    const uint64_t n_chunks = n_events == 0 ? 1 : (n_events + 1023) / 1024;
    return (size_t)n_chunks * R * 8;  // per ping-pong buffer
}

// (chunk, quad word) lanes below which a lane takes ONE repetition instead of four: four times the wavefronts, each a quarter as
// long -- for transcripts that would not fill the chip's wavefront slots otherwise
static uint64_t b3_rpl1_lanes() { return (uint64_t)128 * 1024; }  // (64-repetition shards of the 10^7-gate circuit: digests 0.47 -> 0.38 ms)

// which kernel hashes a byte-row transcript of n chunks (listed: with a quad list of n_quads words; none listed: nothing to launch)
// few lanes (a quarter of the row or less in the verifier; a transcript of a few chunks, i.e. a small circuit):
// one repetition per lane gives four times the wavefronts, each a quarter as long
B3ChunkKernel b3_choose_stream_chunks(uint64_t n, uint32_t NQ, bool listed, uint32_t n_quads, uint32_t batch) {
    if (listed && !n_quads) return B3C_NONE;
    const uint64_t threads = n * (listed ? n_quads : NQ);
    if ((listed && n_quads * 4 <= NQ) || threads * (batch ? batch : 1u) < b3_rpl1_lanes()) return B3C_RPL1;
    if (RV_B3_RPL == 4 && NQ == 64 && !listed) return B3C_UNI;
    return RV_B3_RPL == 4 ? B3C_RPL4 : B3C_RPL1;
}
// does the kernel take rows of NQ quad words?  (a chunk per wavefront: full-width rows and no quad list; bit rows: two quad words a byte)
bool b3_chunk_kernel_takes(B3ChunkKernel k, uint32_t NQ, bool listed, bool bits) {
    if (!NQ || (bits && (NQ & 1 || listed))) return false;
    return k == B3C_RPL1 || k == B3C_RPL4 || (k == B3C_UNI && NQ == 64 && !listed);
}
// chunk chaining values only ([n_chunks][R][8] into d_cv); chunk_base / root_ok: see B_k_b3_chunks
void launch_b3_stream_chunks_as(hipStream_t st, B3ChunkKernel k, const uint32_t* d_stream, uint64_t n_events, uint32_t NQ, uint32_t* d_cv, const uint32_t* d_quads,
                                uint32_t n_quads, uint64_t chunk_base, uint32_t root_ok) {
    const uint64_t n = b3_chunks_of(n_events);
    // (the chaining values of skipped quads stay whatever the scratch buffer held: the tree above them runs on
    // garbage and the caller replaces those digests)
    const uint64_t threads = n * (d_quads ? n_quads : NQ);
    if (k == B3C_NONE) return;
    if (k == B3C_RPL1)
        launch<B_k_b3_chunks<1>, 256>(k_b3_chunks<1>, st, dim3((unsigned)((threads * 4 + 255) / 256)), dim3(256), d_stream, n_events, NQ, n, d_cv, d_quads, n_quads, chunk_base, root_ok);
    else if (k == B3C_UNI)
        launch<B_k_b3_chunks<4, true>, 256>(k_b3_chunks_uni, st, dim3((unsigned)((threads + 255) / 256)), dim3(256), d_stream, n_events, NQ, n, d_cv, d_quads, n_quads, chunk_base, root_ok);
    else
        launch<B_k_b3_chunks<4>, 256>(k_b3_chunks<4>, st, dim3((unsigned)((threads + 255) / 256)), dim3(256), d_stream, n_events, NQ, n, d_cv, d_quads, n_quads, chunk_base, root_ok);
}
void launch_b3_stream_chunks(hipStream_t st, const uint32_t* d_stream, uint64_t n_events, uint32_t NQ, uint32_t* d_cv, const uint32_t* d_quads,
                             uint32_t n_quads, uint64_t chunk_base, uint32_t root_ok) {
    const B3ChunkKernel k = b3_choose_stream_chunks(b3_chunks_of(n_events), NQ, d_quads != nullptr, n_quads, b3_batch_now());
    launch_b3_stream_chunks_as(st, k, d_stream, n_events, NQ, d_cv, d_quads, n_quads, chunk_base, root_ok);
}

uint32_t launch_b3_stream(hipStream_t st, const uint32_t* d_stream, uint64_t n_events, uint32_t NQ, uint32_t* d_cv_a,
                      uint32_t* d_cv_b, uint32_t* d_digest, const uint32_t* d_quads, uint32_t n_quads) {
    const uint32_t R = NQ * 4;
    uint64_t n = n_events == 0 ? 1 : (n_events + 1023) / 1024;
    if (d_quads && !n_quads) return 0;  // a verifier shard without opened repetitions: every online digest comes from the proof
    launch_b3_stream_chunks(st, d_stream, n_events, NQ, d_cv_a, d_quads, n_quads, 0, 1);
    return 1 + b3_reduce_tree(st, d_cv_a, d_cv_b, n, R, d_digest);  // launches
}

// ... and a bit-row transcript (k_b3_chunks_bits1 / k_b3_chunks_bits / k_b3_chunks_bits_uni)
// a transcript of a few chunks (small circuit, and no batch to supply the wavefronts): one repetition per lane
B3ChunkKernel b3_choose_bits_chunks(uint64_t n, uint32_t NQ, uint32_t batch) {
    if (n * NQ * (batch ? batch : 1u) < b3_rpl1_lanes()) return B3C_RPL1;
    return NQ == 64 ? B3C_UNI : B3C_RPL4;
}
void launch_b3_stream_bits_chunks_as(hipStream_t st, B3ChunkKernel k, const uint8_t* d_stream, uint64_t n_events, uint32_t NQ, uint32_t* d_cv, uint64_t chunk_base,
                                     uint32_t root_ok) {
    const uint64_t n = b3_chunks_of(n_events);
    const uint64_t threads = n * NQ;
    if (k == B3C_RPL1)
        launch<B_k_b3_chunks_bits<1>, 256>(k_b3_chunks_bits1, st, dim3((unsigned)((threads * 4 + 255) / 256)), dim3(256), d_stream, n_events, NQ, n,
                                           d_cv, chunk_base, root_ok);
    else if (k == B3C_UNI)
        launch<B_k_b3_chunks_bits<4, true>, 256>(k_b3_chunks_bits_uni, st, dim3((unsigned)((threads + 255) / 256)), dim3(256), d_stream, n_events, NQ, n,
                                                 d_cv, chunk_base, root_ok);
    else
        launch<B_k_b3_chunks_bits<4>, 256>(k_b3_chunks_bits, st, dim3((unsigned)((threads + 255) / 256)), dim3(256), d_stream, n_events, NQ, n,
                                           d_cv, chunk_base, root_ok);
}
void launch_b3_stream_bits_chunks(hipStream_t st, const uint8_t* d_stream, uint64_t n_events, uint32_t NQ, uint32_t* d_cv, uint64_t chunk_base,
                                  uint32_t root_ok) {
    launch_b3_stream_bits_chunks_as(st, b3_choose_bits_chunks(b3_chunks_of(n_events), NQ, b3_batch_now()), d_stream, n_events, NQ, d_cv, chunk_base, root_ok);
}

uint32_t launch_b3_stream_bits(hipStream_t st, const uint8_t* d_stream, uint64_t n_events, uint32_t NQ, uint32_t* d_cv_a,
                           uint32_t* d_cv_b, uint32_t* d_digest) {
    const uint32_t R = NQ * 4;
    const uint64_t n = n_events == 0 ? 1 : (n_events + 1023) / 1024;
    launch_b3_stream_bits_chunks(st, d_stream, n_events, NQ, d_cv_a, 0, 1);
    return 1 + b3_reduce_tree(st, d_cv_a, d_cv_b, n, R, d_digest);  // launches
}

// ---- incremental BLAKE3 tree (streaming prover): the chunk chaining values of a stream arrive in batches ----
// one tree level over a batch: seq = [pending?] ++ in[0 .. n_in); out[i] = parent(seq[2i], seq[2i+1]) for i < n_pairs
// (never ROOT: whether a merge is the root is only known when the stream ends, see k_b3_fold)
__device__ __forceinline__ void b3_pairs_body(const uint32_t* __restrict__ pending, const uint32_t* __restrict__ in, uint64_t n_pairs, uint32_t R,
                                              uint32_t* __restrict__ out) {
    const uint64_t tid = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const uint64_t i = tid / R;
    const uint32_t r = (uint32_t)(tid % R);
    if (i >= n_pairs) return;
    const uint64_t shift = pending ? 1 : 0;
    const uint32_t* lp = (pending && i == 0) ? pending + (size_t)r * 8 : in + ((size_t)(2 * i - shift) * R + r) * 8;
    const uint32_t* rp = in + ((size_t)(2 * i + 1 - shift) * R + r) * 8;
    uint32_t l[8], rr[8], o[8];
#pragma unroll
    for (int k = 0; k < 8; k++) {
        l[k] = lp[k];
        rr[k] = rp[k];
    }
    b3::parent(l, rr, 0, o);
    uint32_t* d = out + ((size_t)i * R + r) * 8;
#pragma unroll
    for (int k = 0; k < 8; k++) d[k] = o[k];
}
__global__ __launch_bounds__(256) void k_b3_pairs(const uint32_t* __restrict__ pending /* [R][8] or null */, const uint32_t* __restrict__ in,
                                                  uint64_t n_pairs, uint32_t R, uint32_t* __restrict__ out) {
    b3_pairs_body(pending, in, n_pairs, R, out);
}
// the same tree level for up to B3PairsBatch::MAX streams of equal shape at once: blockIdx.y = stream (a batch stream's proofs)
__global__ __launch_bounds__(256) void k_b3_pairs_batched(B3PairsBatch L, uint64_t n_pairs, uint32_t R) {
    const uint32_t y = blockIdx.y;
    b3_pairs_body(L.pending[y], L.in[y], n_pairs, R, L.out[y]);
}
void launch_b3_pairs_batched(hipStream_t st, const B3PairsBatch& L, uint64_t n_pairs, uint32_t R) {
    if (!n_pairs || !L.n) return;
    const uint64_t threads = n_pairs * R;
    hipLaunchKernelGGL(k_b3_pairs_batched, dim3((unsigned)((threads + 255) / 256), L.n), dim3(256), 0, st, L, n_pairs, R);
}
void launch_b3_pairs(hipStream_t st, const uint32_t* d_pending, const uint32_t* d_in, uint64_t n_pairs, uint32_t R, uint32_t* d_out) {
    if (!n_pairs) return;
    const uint64_t threads = n_pairs * R;
    hipLaunchKernelGGL(k_b3_pairs, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, st, d_pending, d_in, n_pairs, R, d_out);
}
// end of a stream: the last chunk's chaining value folded into the pending subtree roots, smallest first; the last
// merge is the root (a lone last chunk was hashed with ROOT already and n = 0 just copies it)
__global__ void k_b3_fold(B3FoldList L, const uint32_t* __restrict__ last, uint32_t R, uint32_t* __restrict__ digest) {
    const uint32_t r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= R) return;
    uint32_t cv[8];
#pragma unroll
    for (int k = 0; k < 8; k++) cv[k] = last[(size_t)r * 8 + k];
    for (uint32_t i = 0; i < L.n; i++) {
        uint32_t l[8], o[8];
#pragma unroll
        for (int k = 0; k < 8; k++) l[k] = L.p[i][(size_t)r * 8 + k];
        b3::parent(l, cv, i + 1 == L.n ? b3::ROOT : 0u, o);
#pragma unroll
        for (int k = 0; k < 8; k++) cv[k] = o[k];
    }
#pragma unroll
    for (int k = 0; k < 8; k++) digest[(size_t)r * 8 + k] = cv[k];
}
void launch_b3_fold(hipStream_t st, const B3FoldList& L, const uint32_t* d_last, uint32_t R, uint32_t* d_digest) {
    hipLaunchKernelGGL(k_b3_fold, dim3((R + 63) / 64), dim3(64), 0, st, L, d_last, R, d_digest);
}

// Transcript::hash + CombineInstance::hash: h = B3(B3(pre2||on2) || B3(pre64||on64))
struct B_k_join {
    __device__ __forceinline__ void operator()(const uint32_t* __restrict__ pre2, const uint32_t* __restrict__ on2, const uint32_t* __restrict__ pre64, const uint32_t* __restrict__ on64, uint32_t R, uint8_t* __restrict__ h) const {
    const uint32_t r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= R) return;
    uint32_t m[16], h2[8], h64[8], o[8];
#pragma unroll
    for (int k = 0; k < 8; k++) {
        m[k] = pre2[r * 8 + k];
        m[8 + k] = on2[r * 8 + k];
    }
    b3::hash64(m, h2);
#pragma unroll
    for (int k = 0; k < 8; k++) {
        m[k] = pre64[r * 8 + k];
        m[8 + k] = on64[r * 8 + k];
    }
    b3::hash64(m, h64);
#pragma unroll
    for (int k = 0; k < 8; k++) {
        m[k] = h2[k];
        m[8 + k] = h64[k];
    }
    b3::hash64(m, o);
    uint32_t* d = (uint32_t*)(h + 32 * (size_t)r);
#pragma unroll
    for (int k = 0; k < 8; k++) d[k] = o[k];
}
};
__global__ void k_join(const uint32_t* __restrict__ pre2, const uint32_t* __restrict__ on2, const uint32_t* __restrict__ pre64, const uint32_t* __restrict__ on64, uint32_t R, uint8_t* __restrict__ h) {
    B_k_join{}(pre2, on2, pre64, on64, R, h);
}

void launch_join(hipStream_t st, const uint32_t* d_pre2, const uint32_t* d_on2, const uint32_t* d_pre64, const uint32_t* d_on64,
                 uint32_t R, uint8_t* d_h) {
    launch<B_k_join, 64>(k_join, st, dim3((R + 63) / 64), dim3(64), d_pre2, d_on2, d_pre64, d_on64, R, d_h);
}

}  // namespace rv
