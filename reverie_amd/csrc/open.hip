// Fiat-Shamir, openings and their inverse for gfx950: the verifier's set-up kernels, the challenge, extraction of the opened
// repetitions' vectors, unpacking them again, the record heads and the early-corrections path.
// (The interpreter: interp.hip; the transcript hashes the challenge is drawn from: b3_tree.hip.)
//
// Replaces (all under the reference's src/):
//   transcript/prover.rs:57-175 + algebra/gf2/{share,recon}.rs Pack/PackSelected  (openings)
//   proof/mod.rs:68-108, crypto/ro.rs:8-20                     combine_hashes, RandomOracle, challenge_to_opening
#include <algorithm>

#include "b3.h"
#include "gf2dev.h"
#include "internal.h"
#include "launch.h"

namespace rv {

// verifier set-up: rows of `src` replace those of `dst` for the repetitions with (omit[r] < 8) == want_online
// (opened player keys and carried-over online commitments arrive in ONE staging copy instead of one tiny
// host-to-device copy per repetition)
struct B_k_overlay_rows {
    __device__ __forceinline__ void operator()(uint32_t* __restrict__ dst, const uint32_t* __restrict__ src, const uint8_t* __restrict__ omit, uint32_t R, uint32_t row_words, int want_online) const {
    const uint32_t r = blockIdx.x;
    if (r >= R || (int)(omit[r] < RV_PLAYERS) != want_online) return;
    for (uint32_t t = threadIdx.x; t < row_words; t += blockDim.x) dst[(size_t)r * row_words + t] = src[(size_t)r * row_words + t];
}
};
__global__ void k_overlay_rows(uint32_t* __restrict__ dst, const uint32_t* __restrict__ src, const uint8_t* __restrict__ omit, uint32_t R, uint32_t row_words, int want_online) {
    B_k_overlay_rows{}(dst, src, omit, R, row_words, want_online);
}

// parity hook for DomainGF2::reconstruct (gf2/domain.rs:47-63): the reference's packed u64 share is two quad words (hi, lo)
__global__ void k_hook_recon_gf2(const uint64_t* __restrict__ shares, uint64_t n, uint64_t* __restrict__ out) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint64_t v = shares[i];
    out[i] = ((uint64_t)recon32((uint32_t)(v >> 32)) << 32) | recon32((uint32_t)v);
}
void launch_hook_recon_gf2(hipStream_t st, const uint64_t* d_shares, uint64_t n, uint64_t* d_out) {
    if (n) hipLaunchKernelGGL(k_hook_recon_gf2, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, d_shares, n, d_out);
}

void launch_overlay_rows(hipStream_t st, uint32_t* d_dst, const uint32_t* d_src, const uint8_t* d_omit, uint32_t R,
                         uint32_t row_words, int want_online) {
    launch<B_k_overlay_rows, 32>(k_overlay_rows, st, dim3(R), dim3(32), d_dst, d_src, d_omit, R, row_words, want_online);
}

// n_rows copies of one 32-byte digest (the Z64 transcripts of a pure GF(2) circuit are empty: BLAKE3(""))
struct Digest8 {
    uint32_t w[8];
};
struct B_k_fill_digests {
    __device__ __forceinline__ void operator()(uint32_t* __restrict__ dst, uint32_t n_rows, Digest8 d) const {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n_rows * 8) dst[i] = d.w[i & 7];
}
};
__global__ void k_fill_digests(uint32_t* __restrict__ dst, uint32_t n_rows, Digest8 d) {
    B_k_fill_digests{}(dst, n_rows, d);
}
void launch_fill_digests(hipStream_t st, uint32_t* d_dst, uint32_t n_rows, const uint32_t digest[8]) {
    Digest8 d;
    for (int k = 0; k < 8; k++) d.w[k] = digest[k];
    launch<B_k_fill_digests, 256>(k_fill_digests, st, dim3((n_rows * 8 + 255) / 256), dim3(256), d_dst, n_rows, d);
}

// start of the interpreter phase: clear the invalid-witness flag and the all-zero row (mask words, corr-bit words)
// (fill / n_fill_rows / d: also n_fill_rows copies of the digest d -- the Z64 transcripts' digests of a pure GF(2) circuit, BLAKE3(""),
// which otherwise cost a launch of their own between the hashes and the commitment)
struct B_k_shard_init {
    __device__ __forceinline__ void operator()(int* __restrict__ err, uint32_t* __restrict__ zero_mask, uint32_t n_mask_words, uint8_t* __restrict__ zero_corr, uint32_t n_corr_bytes,
                                               uint32_t* __restrict__ fill, uint32_t n_fill_rows, Digest8 d, uint8_t* __restrict__ zero_byte) const {
    const uint32_t i = threadIdx.x;
    if (i == 0) *err = 0;
    if (i == 1 && zero_byte) *zero_byte = 0;  // (MODE_PROVE_V: the zero row's cleartext value -- a memset launch of its own before)
    if (i < n_mask_words) zero_mask[i] = 0;
    if (i < n_corr_bytes) zero_corr[i] = 0;
    if (fill)
        for (uint32_t j = i; j < n_fill_rows * 8; j += blockDim.x) fill[j] = d.w[j & 7];
}
};
__global__ void k_shard_init(int* __restrict__ err, uint32_t* __restrict__ zero_mask, uint32_t n_mask_words, uint8_t* __restrict__ zero_corr, uint32_t n_corr_bytes,
                             uint32_t* __restrict__ fill, uint32_t n_fill_rows, Digest8 d, uint8_t* __restrict__ zero_byte) {
    B_k_shard_init{}(err, zero_mask, n_mask_words, zero_corr, n_corr_bytes, fill, n_fill_rows, d, zero_byte);
}
void launch_shard_init(hipStream_t st, int* d_err, uint32_t* d_zero_mask, uint32_t n_mask_words, uint8_t* d_zero_corr,
                       uint32_t n_corr_bytes, uint32_t* d_fill, uint32_t n_fill_rows, const uint32_t* digest, uint8_t* d_zero_byte) {
    Digest8 d{};
    if (d_fill)
        for (int k = 0; k < 8; k++) d.w[k] = digest[k];
    launch<B_k_shard_init, 64>(k_shard_init, st, dim3(1), dim3(64), d_err, d_zero_mask, n_mask_words, d_zero_corr, n_corr_bytes, d_fill, n_fill_rows, d, d_zero_byte);
}

// ------------------------------------------------------------------------------------
// Openings.  kind 0: omitted player's bit of a recorded broadcast share (PackSelected,
// gf2/share.rs:87-149); kind 1: a 0x00/0xFF recon byte (Pack, gf2/recon.rs:189-239).
// Items are packed 8 per byte MSB-first; the output vector has n_items/8 + 1 bytes (the
// reference always emits one more chunk).
//
// A workgroup produces EX_TB consecutive output bytes of EVERY opened repetition: the packed
// bytes are first collected in LDS ([slot][byte]) and then written out as contiguous runs.
// (Writing each byte straight from the lane that computed it cost 40 single-byte partial-line
// writes per 16 lines read: the kernel was bound by write transactions, not by HBM bytes.)
// ------------------------------------------------------------------------------------
constexpr uint32_t EX_TB = 128;
// (k_extract_rows: its own tile, for A/B builds)
#ifndef RV_EXR_TB
#define RV_EXR_TB 256
#endif
constexpr uint32_t EXR_TB = RV_EXR_TB;

// slot of every opened repetition (rank among the opened ones) and its output offset, into LDS
__device__ __forceinline__ uint32_t ex_slots(const uint8_t* __restrict__ omit, const uint64_t* __restrict__ dst_off, uint32_t R,
                                             uint8_t* s_slot /*[256]*/, uint64_t* s_dst /*[RV_ONLINE_REPS]*/, uint32_t* s_cnt /*[5]*/) {
    const uint32_t tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const bool on = tid < R && omit[tid] < 8;
    const unsigned long long bal = __ballot(on);
    if (lane == 0) s_cnt[wave] = (uint32_t)__popcll(bal);
    __syncthreads();
    uint32_t base = 0;
    for (uint32_t w = 0; w < wave; w++) base += s_cnt[w];
    const uint32_t slot = base + (uint32_t)__popcll(bal & ((1ull << lane) - 1ull));
    s_slot[tid] = (on && slot < RV_ONLINE_REPS) ? (uint8_t)slot : (uint8_t)0xFF;
    if (on && slot < RV_ONLINE_REPS) s_dst[slot] = dst_off[tid];
    uint32_t n = 0;
    for (uint32_t w = 0; w < 4; w++) n += s_cnt[w];
    __syncthreads();
    return n < RV_ONLINE_REPS ? n : RV_ONLINE_REPS;
}

// contiguous write-out of the collected bytes: s_buf[slot][0 .. nb)
template <uint32_t TB = EX_TB>
__device__ __forceinline__ void ex_flush(const uint8_t* s_buf, const uint64_t* s_dst, uint32_t n_slots, uint64_t t0, uint32_t nb,
                                         uint8_t* __restrict__ out, uint32_t k0 = 0) {
    for (uint32_t idx = threadIdx.x + k0 * TB; idx < n_slots * TB; idx += blockDim.x) {
        const uint32_t k = idx / TB, i = idx % TB;
        if (i < nb && s_dst[k] != ~0ull) out[s_dst[k] + t0 + i] = s_buf[k * TB + i];  // (~0: a slot that is left out)
    }
}

// the same to page-locked HOST memory (internal.h: OpenDirect), in whole 16-byte aligned words: every word that STARTS inside the
// slot's run of nb bytes and ends inside the nbx >= nb bytes the workgroup has extracted (a run starts at an odd offset of the proof;
// byte stores cross the link as partial writes one by one, and with them the proof was SLOWER than without the direct path).  What is
// left -- the partial words at a vector's two ends -- k_copy_gaps copies from the image.  `out` is 16-byte aligned; TB = the stride
// of s_buf.
template <uint32_t TB>
__device__ __forceinline__ void ex_flush_host(const uint8_t* s_buf, const uint64_t* s_dst, uint32_t n_slots, uint64_t t0, uint32_t nb, uint32_t nbx,
                                              uint8_t* __restrict__ out) {
    constexpr uint32_t W = TB / 16 + 1;
    for (uint32_t idx = threadIdx.x; idx < n_slots * W; idx += blockDim.x) {
        const uint32_t k = idx / W, w = idx % W;
        if (s_dst[k] == ~0ull) continue;
        const uint64_t d0 = s_dst[k] + t0;
        const uint64_t wa = (d0 & ~15ull) + 16ull * w;
        if (wa >= d0 + nb) continue;
        const uint8_t* sp = s_buf + k * TB;
        if (wa >= d0 && wa + 16 <= d0 + nbx) {
            const uint32_t o = (uint32_t)(wa - d0);
            uint32_t x[4];
#pragma unroll
            for (int q = 0; q < 4; q++)
                x[q] = (uint32_t)sp[o + 4 * q] | ((uint32_t)sp[o + 4 * q + 1] << 8) | ((uint32_t)sp[o + 4 * q + 2] << 16) | ((uint32_t)sp[o + 4 * q + 3] << 24);
            *(uint4*)(out + wa) = make_uint4(x[0], x[1], x[2], x[3]);
        }
    }
}

template <int KIND>
struct B_k_extract_rows {
    // block0: added to blockIdx.x modulo 2^32 = this launch's workgroup 0 is workgroup block0 of the vectors (k_open_small runs the
    // extraction as one range of its grid and passes minus the range's first workgroup)
    __device__ __forceinline__ void operator()(const uint32_t* __restrict__ stream, const uint32_t* __restrict__ rows, uint64_t n_items, uint32_t NQ, uint32_t tb /* <= EXR_TB */, const uint8_t* __restrict__ omit /*[R]*/, const uint64_t* __restrict__ dst_off /*[R]*/, uint8_t* __restrict__ out, uint32_t block0, uint8_t* __restrict__ out2 = nullptr, uint32_t n_direct = 0) const {
    // (internal.h: OpenDirect) a workgroup that also writes to the proof buffer on the host sends every 16-byte aligned word that
    // STARTS in its tile, so it extracts up to LA bytes of the next tile as well: no word is left for two workgroups to share
    constexpr uint32_t LA = 16, SB = EXR_TB + LA;
    __shared__ uint8_t s_buf[RV_ONLINE_REPS * SB];
    __shared__ uint32_t s_rows[8 * SB];
    __shared__ uint8_t s_slot[256];
    __shared__ uint64_t s_dst[RV_ONLINE_REPS];
    __shared__ uint32_t s_cnt[4];
    __shared__ uint8_t s_aq[64];
    __shared__ uint32_t s_naq;
    const uint64_t n_bytes = n_items / 8 + 1;
    const uint64_t t0 = (uint64_t)(uint32_t)(blockIdx.x + block0) * tb;  // (modulo 2^32: k_open_small passes minus its range's first block)
    const uint32_t nb = (uint32_t)((n_bytes - t0 < tb) ? n_bytes - t0 : tb);
    const bool direct = out2 && blockIdx.x + block0 < n_direct;
    const uint32_t nbx = direct ? (uint32_t)((n_bytes - t0 < nb + LA) ? n_bytes - t0 : nb + LA) : nb;  // bytes extracted
    // this workgroup's row ids, one coalesced pass (ordinals past the end repeat the last item; masked below)
    for (uint32_t i = threadIdx.x; i < 8 * nbx; i += 256) {
        uint64_t it = 8 * t0 + i;
        if (it >= n_items) it = n_items ? n_items - 1 : 0;
        s_rows[i] = rows ? rows[it] : (uint32_t)it;
    }
    const uint32_t n_slots = ex_slots(omit, dst_off, 4 * NQ, s_slot, s_dst, s_cnt);  // contains the barrier for s_rows
    if (!n_slots) return;
    // the quad words that hold an opened repetition (about 30 of 64 for a whole proof), compacted: thread = (output byte,
    // such a quad), so no lane idles on a quad nobody opened (k_extract_rows<0> 263 -> 240 us on the 10^7-gate circuit)
    if (threadIdx.x < 64) {
        const uint32_t q = threadIdx.x;
        bool act = false;
        if (q < NQ) {
#pragma unroll
            for (int i = 0; i < 4; i++) {
                act |= s_slot[4 * q + i] != 0xFF;
            }
        }
        const unsigned long long bal = __ballot(act);
        if (act) s_aq[__popcll(bal & ((1ull << q) - 1ull))] = (uint8_t)q;
        if (q == 0) s_naq = (uint32_t)__popcll(bal);
    }
    __syncthreads();
    const uint32_t n_aq = s_naq;
    if (!n_aq) return;
    const uint32_t dtl = 256 / n_aq, da = 256 % n_aq;
    for (uint32_t tl = threadIdx.x / n_aq, a = threadIdx.x % n_aq; tl < nbx;) {
        const uint32_t q = s_aq[a];
        uint32_t sl[4], om[4];
#pragma unroll
        for (int i = 0; i < 4; i++) {
            sl[i] = s_slot[4 * q + i];
            om[i] = omit[4 * q + i];
        }
        const uint64_t it0 = 8 * (t0 + tl);
        uint32_t w[8];
        // (read once: nontemporal, 0.43 -> 0.41 ms for the opening phase)
#pragma unroll
        for (int j = 0; j < 8; j++) w[j] = n_items ? __builtin_nontemporal_load(&stream[(size_t)s_rows[8 * tl + j] * NQ + q]) : 0u;
        // rows past the end contribute zero bits (their loads were clamped to the last item)
#pragma unroll
        for (int j = 0; j < 8; j++)
            if (it0 + j >= n_items) w[j] = 0;
        // only the opened repetitions of the quad (usually one of the four) are worth the bit gathering
#pragma unroll
        for (int i = 0; i < 4; i++) {
            if (sl[i] == 0xFF) continue;
            const uint32_t sh = (KIND == 0) ? (31u - 8u * i - (om[i] & 7u)) : (24u - 8u * i);
            uint32_t acc = 0;
#pragma unroll
            for (int j = 0; j < 8; j++) acc |= ((w[j] >> sh) & 1u) << (7 - j);
            s_buf[sl[i] * SB + tl] = (uint8_t)acc;
        }
        a += da;
        tl += dtl;
        if (a >= n_aq) {
            a -= n_aq;
            tl++;
        }
    }
    __syncthreads();
    ex_flush<SB>(s_buf, s_dst, n_slots, t0, nb, out);
    if (direct) ex_flush_host<SB>(s_buf, s_dst, n_slots, t0, nb, nbx, out2);
}
};
template <int KIND>
__global__ __launch_bounds__(256) void k_extract_rows(const uint32_t* __restrict__ stream, const uint32_t* __restrict__ rows, uint64_t n_items, uint32_t NQ, uint32_t tb /* <= EX_TB */, const uint8_t* __restrict__ omit /*[R]*/, const uint64_t* __restrict__ dst_off /*[R]*/, uint8_t* __restrict__ out, uint32_t block0, uint8_t* __restrict__ out2, uint32_t n_direct) {
    B_k_extract_rows<KIND>{}(stream, rows, n_items, NQ, tb, omit, dst_off, out, block0, out2, n_direct);
}

// Bit-per-rep source (the preprocessing stream, [n][NQ/2] bytes; nibble bit k of quad q <-> repetition 4q+3-k):
// the workgroup's 8*tb rows are contiguous in HBM and are copied to LDS in one coalesced pass; thread =
// (output byte, opened repetition) then picks its 8 bits out of LDS.
struct B_k_extract_from_bits {
    // (block0: added to blockIdx.x modulo 2^32 -- k_open_small runs this as one range of its grid)
    __device__ __forceinline__ void operator()(const uint8_t* __restrict__ bits, uint64_t n_items, uint32_t NQ, uint32_t tb /* <= EX_TB */, const OnlineList* __restrict__ olp, uint8_t* __restrict__ out, uint32_t rep_min, uint32_t block0 = 0) const {
    __shared__ uint8_t s_buf[RV_ONLINE_REPS * EX_TB];
    __shared__ uint64_t s_dst[RV_ONLINE_REPS];
    __shared__ uint32_t s_pos[RV_ONLINE_REPS];  // byte in the row << 3 | bit in the byte
    __shared__ __attribute__((aligned(16))) uint8_t s_pre[8 * EX_TB * 32];
    const uint32_t n_ol = olp->n < RV_ONLINE_REPS ? olp->n : RV_ONLINE_REPS;
    if (!n_ol) return;
    const uint64_t n_bytes = n_items / 8 + 1;
    const uint64_t t0 = (uint64_t)(uint32_t)(blockIdx.x + block0) * tb;
    const uint32_t nb = (uint32_t)((n_bytes - t0 < tb) ? n_bytes - t0 : tb);
    const uint32_t h = NQ >> 1;  // bytes per row
    const uint64_t r0 = 8 * t0;
    const uint32_t n_rows = (uint32_t)(r0 >= n_items ? 0 : (n_items - r0 < 8ull * nb ? n_items - r0 : 8ull * nb));
    const uint8_t* src = bits + r0 * h;  // 8-byte aligned (r0 is a multiple of 8); 16-byte when h is even
    const uint32_t total = n_rows * h;
    if ((h & 1) == 0) {
        for (uint32_t i = threadIdx.x * 16; i + 16 <= total; i += 256 * 16) *(uint4*)(s_pre + i) = *(const uint4*)(src + i);
        for (uint32_t i = (total & ~15u) + threadIdx.x; i < total; i += 256) s_pre[i] = src[i];
    } else {
        for (uint32_t i = threadIdx.x; i < total; i += 256) s_pre[i] = src[i];
    }
    if (threadIdx.x < n_ol) {
        const uint32_t r = olp->rep[threadIdx.x];
        s_dst[threadIdx.x] = r < rep_min ? ~0ull : olp->dst[threadIdx.x];  // (early corrections: the host has the vectors of the repetitions below rep_min)
        s_pos[threadIdx.x] = ((r >> 3) << 3) | (4 * ((r >> 2) & 1) + 3 - (r & 3));
    }
    __syncthreads();
    // thread = (opened repetition k, output-byte lane): k, and with it the byte / bit it picks out of a row, stay in
    // registers for the whole loop (an index split per output byte cost 4x the instructions: 123 -> 45 us per proof)
    {
        const uint32_t lanes = 256 / n_ol;  // output bytes in flight per repetition
        const uint32_t k = threadIdx.x % n_ol, tlane = threadIdx.x / n_ol;
        if (tlane < lanes) {
            const uint32_t pos = s_pos[k], bit = pos & 7;
            const uint8_t* col = s_pre + (pos >> 3);
            const uint32_t full = n_rows / 8;  // output bytes whose eight rows all exist
            for (uint32_t tl = tlane; tl < nb; tl += lanes) {
                uint32_t acc = 0;
                if (tl < full) {
#pragma unroll
                    for (int j = 0; j < 8; j++) acc |= (((uint32_t)col[(8 * tl + j) * h] >> bit) & 1u) << (7 - j);
                } else {
                    for (uint32_t j = 0; j < 8; j++)
                        if (8 * tl + j < n_rows) acc |= (((uint32_t)col[(8 * tl + j) * h] >> bit) & 1u) << (7 - j);
                }
                s_buf[k * EX_TB + tl] = (uint8_t)acc;
            }
        }
    }
    __syncthreads();
    ex_flush(s_buf, s_dst, n_ol, t0, nb, out);
}
};
__global__ __launch_bounds__(256) void k_extract_from_bits(const uint8_t* __restrict__ bits, uint64_t n_items, uint32_t NQ, uint32_t tb /* <= EX_TB */, const OnlineList* __restrict__ olp, uint8_t* __restrict__ out, uint32_t rep_min) {
    B_k_extract_from_bits{}(bits, n_items, NQ, tb, olp, out, rep_min);
}

static uint32_t ex_tb_for(uint64_t n_bytes, uint32_t cap = EX_TB) {
    // output bytes per workgroup: the full EX_TB when that still yields several workgroups per CU, fewer for
    // short vectors (a workgroup walks its bytes in a serial loop)
    uint32_t tb = cap;
    while (tb > 8 && (n_bytes + tb - 1) / tb < 2048) tb /= 2;
    return tb;
}

void launch_extract_from_bits(hipStream_t st, const uint8_t* d_bits, uint64_t n_items, uint32_t NQ, const OnlineList* d_ol,
                              uint8_t* d_out, uint32_t rep_min) {
    const uint64_t n_bytes = n_items / 8 + 1;
    const uint32_t tb = ex_tb_for(n_bytes);
    launch<B_k_extract_from_bits, 256>(k_extract_from_bits, st, dim3((unsigned)((n_bytes + tb - 1) / tb)), dim3(256), d_bits, n_items, NQ, tb, d_ol,
                       d_out, rep_min);
}

// ------------------------------------------------------------------------------------
// Fiat-Shamir on the device (one wavefront).  combine_hashes (proof/mod.rs:102-108): comm =
// BLAKE3 of the 256 digests = 8 chunks (lanes 0..7, 16 chained compressions each) + a 3-level
// tree.  RandomOracle (crypto/ro.rs:8-20) + challenge_to_opening (proof/mod.rs:68-83): XOF of
// "random-oracle challenge" || 0x00 || comm; 16-byte draws, u128 LE mod 256 then mod 8 = the
// first byte of each draw; every lane produces one 64-byte XOF block = two (rep, omit) pairs,
// lane 0 replays them in order (a re-drawn repetition overwrites its omit) until 40 distinct.
// ------------------------------------------------------------------------------------
// The shard form (rep_begin, R): h holds ALL 256 digests (after the all-gather they are on every GPU), the challenge is
// derived for all repetitions, and the offsets / OnlineList / omit[0..R) are produced for the shard's own repetitions.
// How many of them are opened is only known here, so the section starts (online records, then preprocessing records,
// per domain) are computed on the device from L.base[0] (= start of the output, 40 past it when framed) and returned
// in res = {n_online_local, n_preprocessing_local}; omit_all (nullable) receives the full map for the host.
struct B_k_fs_challenge {
    __device__ __forceinline__ void operator()(const uint8_t* __restrict__ h, FsLayout L, uint32_t rep_begin, uint32_t R, uint8_t* __restrict__ comm, uint8_t* __restrict__ omit, uint8_t* __restrict__ omit_all, uint64_t* __restrict__ offs, OnlineList* __restrict__ ol, uint32_t* __restrict__ res, uint32_t* __restrict__ mbox = nullptr, uint32_t* __restrict__ mbox_flag = nullptr, uint32_t mbox_seq = 0) const {
    __shared__ uint32_t s_cv[8][8], s_t1[4][8], s_t2[2][8], s_comm[8];
    __shared__ uint32_t s_msg[16];
    __shared__ uint8_t s_draw[128][2];
    __shared__ uint8_t s_omit[RV_TOTAL_REPS];
    __shared__ uint32_t s_count;
    const uint32_t lane = threadIdx.x;
    const uint32_t* hw = (const uint32_t*)h;
    // The commitment's 8 chunks x 16 chained blocks and its three tree levels are 19 compressions one after the other on the path
    // between the hashes and the openings of EVERY proof: a quad of lanes per compression (b3.h: compress_q, the digests staged in
    // LDS for the quads to share) instead of a lane -- 41 -> about 25 us for the kernel.
    __shared__ uint32_t s_h[RV_TOTAL_REPS * 8];
#pragma unroll
    for (uint32_t i = 0; i < RV_TOTAL_REPS * 8 / 64; i++) s_h[i * 64 + lane] = hw[i * 64 + lane];
    for (uint32_t r = lane; r < RV_TOTAL_REPS; r += 64) s_omit[r] = RV_PLAYERS;
    if (lane == 0) s_count = 0;
    __syncthreads();
    const uint32_t qc = lane & 3, qi = lane >> 2;  // column, quad
    const b3::QuadSchedule qs = b3::quad_schedule(qc);
    const uint32_t iv_a = qc == 0 ? B3_IV0 : qc == 1 ? B3_IV1 : qc == 2 ? B3_IV2 : B3_IV3;
    const uint32_t iv_b = qc == 0 ? B3_IV4 : qc == 1 ? B3_IV5 : qc == 2 ? B3_IV6 : B3_IV7;
    {
        // (all 16 quads run -- quad_from moves data between the lanes of a quad, every lane must be active --, the first 8 count)
        const uint32_t ch = qi & 7;
        uint32_t cva = iv_a, cvb = iv_b;
        for (uint32_t b = 0; b < 16; b++)
            b3::compress_q<false>(cva, cvb, s_h + ch * 256 + b * 16, qs, qc, ch, 64, (b == 0 ? b3::CHUNK_START : 0u) | (b == 15 ? b3::CHUNK_END : 0u));
        if (qi < 8) s_cv[qi][qc] = cva, s_cv[qi][4 + qc] = cvb;
    }
    __syncthreads();
    {
        uint32_t cva = iv_a, cvb = iv_b;
        b3::compress_q<false>(cva, cvb, &s_cv[2 * (qi & 3)][0], qs, qc, 0, 64, b3::PARENT);  // (s_cv[2p], s_cv[2p + 1]: 16 consecutive words)
        if (qi < 4) s_t1[qi][qc] = cva, s_t1[qi][4 + qc] = cvb;
    }
    __syncthreads();
    {
        uint32_t cva = iv_a, cvb = iv_b;
        b3::compress_q<false>(cva, cvb, &s_t1[2 * (qi & 1)][0], qs, qc, 0, 64, b3::PARENT);
        if (qi < 2) s_t2[qi][qc] = cva, s_t2[qi][4 + qc] = cvb;
    }
    __syncthreads();
    {
        uint32_t cva = iv_a, cvb = iv_b;
        b3::compress_q<false>(cva, cvb, &s_t2[0][0], qs, qc, 0, 64, b3::PARENT | b3::ROOT);
        if (qi == 0) s_comm[qc] = cva, s_comm[4 + qc] = cvb;
    }
    __syncthreads();
    if (lane == 0) {
        // the random oracle's one input block: context string, a zero byte, comm; 56 bytes, zero padded
        const char ctx[] = "random-oracle challenge";  // proof/mod.rs:18
        uint8_t blk[64];
        for (int i = 0; i < 64; i++) blk[i] = 0;
        for (int i = 0; i < 23; i++) blk[i] = (uint8_t)ctx[i];
        for (int i = 0; i < 8; i++) {
            comm[4 * i + 0] = blk[24 + 4 * i + 0] = (uint8_t)(s_comm[i]);
            comm[4 * i + 1] = blk[24 + 4 * i + 1] = (uint8_t)(s_comm[i] >> 8);
            comm[4 * i + 2] = blk[24 + 4 * i + 2] = (uint8_t)(s_comm[i] >> 16);
            comm[4 * i + 3] = blk[24 + 4 * i + 3] = (uint8_t)(s_comm[i] >> 24);
            if (L.comm2) {
                L.comm2[4 * i + 0] = (uint8_t)(s_comm[i]);
                L.comm2[4 * i + 1] = (uint8_t)(s_comm[i] >> 8);
                L.comm2[4 * i + 2] = (uint8_t)(s_comm[i] >> 16);
                L.comm2[4 * i + 3] = (uint8_t)(s_comm[i] >> 24);
            }
        }
        for (int i = 0; i < 16; i++)
            s_msg[i] = (uint32_t)blk[4 * i] | ((uint32_t)blk[4 * i + 1] << 8) | ((uint32_t)blk[4 * i + 2] << 16) |
                       ((uint32_t)blk[4 * i + 3] << 24);
    }
    __syncthreads();
    uint32_t m[16], cv[8];
#pragma unroll
    for (int k = 0; k < 16; k++) m[k] = s_msg[k];
    b3::iv(cv);
    for (uint64_t base = 0;; base += 64) {
        uint32_t o[16];
        b3::compress<true>(cv, m, base + lane, 56, b3::CHUNK_START | b3::CHUNK_END | b3::ROOT, o);
        s_draw[2 * lane][0] = (uint8_t)o[0];
        s_draw[2 * lane][1] = (uint8_t)(o[4] & 7u);
        s_draw[2 * lane + 1][0] = (uint8_t)o[8];
        s_draw[2 * lane + 1][1] = (uint8_t)(o[12] & 7u);
        __syncthreads();
        if (lane == 0) {
            uint32_t count = s_count;
            for (uint32_t i = 0; i < 128 && count < RV_ONLINE_REPS; i++) {
                const uint32_t rep = s_draw[i][0];
                if (s_omit[rep] == RV_PLAYERS) count++;
                s_omit[rep] = s_draw[i][1];
            }
            s_count = count;
        }
        __syncthreads();
        if (s_count >= RV_ONLINE_REPS) break;
    }
    // offsets of every repetition's record and of its vectors (the same arithmetic as the host path)
    if (omit_all)
        for (uint32_t r = lane; r < RV_TOTAL_REPS; r += 64) omit_all[r] = s_omit[r];
    uint32_t n_on = 0;  // opened repetitions of this shard
    for (uint32_t c = 0; c < (R + 63) / 64; c++) {
        const uint32_t r = 64 * c + lane;
        n_on += (uint32_t)__popcll(__ballot(r < R && s_omit[rep_begin + r] < RV_PLAYERS));
    }
    const uint32_t n_pre = R - n_on;
    // sections: [gf2 online | gf2 preprocessing | z64 online | z64 preprocessing]; when the caller frames the
    // output as bincode(Proof) (single shard) L.base[] already holds the four starts, otherwise only base[0] counts
    uint64_t base[4];
    if (L.framed) {
#pragma unroll
        for (int k = 0; k < 4; k++) base[k] = L.base[k];
    } else {
        base[0] = L.base[0];
        base[1] = base[0] + (uint64_t)n_on * L.sz2;
        base[2] = base[1] + (uint64_t)n_pre * 48;
        base[3] = base[2] + (uint64_t)n_on * L.sz64;
    }
    uint32_t k_on = 0, k_pre = 0;
    for (uint32_t c = 0; c < (R + 63) / 64; c++) {
        const uint32_t r = 64 * c + lane;
        const bool valid = r < R;
        const uint32_t om = valid ? s_omit[rep_begin + r] : RV_PLAYERS;
        const bool on = valid && om < RV_PLAYERS;
        const unsigned long long bal = __ballot(on), val = __ballot(valid);
        const unsigned long long lt = (1ull << lane) - 1ull;
        const uint32_t my_on = k_on + (uint32_t)__popcll(bal & lt), my_pre = k_pre + (uint32_t)__popcll(~bal & val & lt);
        if (valid) {
            omit[r] = (uint8_t)om;
            uint64_t v[8] = {0, 0, 0, 0, 0, 0, 0, 0};
            if (on) {
                v[0] = base[0] + (uint64_t)my_on * L.sz2;
                v[1] = base[2] + (uint64_t)my_on * L.sz64;
                v[2] = v[0] + 137;
                v[3] = v[0] + 145 + L.l2r;
                v[4] = v[0] + 153 + L.l2r + L.l2c;
                v[5] = v[1] + 137;
                v[6] = v[1] + 145 + L.l64r;
                v[7] = v[1] + 153 + L.l64r + L.l64c;
                if (my_on < RV_ONLINE_REPS) {
                    ol->rep[my_on] = r;
                    ol->dst[my_on] = v[3];
                }
            } else {
                v[0] = base[1] + (uint64_t)my_pre * 48;
                v[1] = base[3] + (uint64_t)my_pre * 48;
            }
#pragma unroll
            for (int j = 0; j < 8; j++) offs[(size_t)j * R + r] = v[j];
        }
        k_on += (uint32_t)__popcll(bal);
        k_pre += (uint32_t)__popcll(~bal & val);
    }
    if (lane == 0) {
        ol->n = n_on < RV_ONLINE_REPS ? n_on : RV_ONLINE_REPS;
        if (res) {
            res[0] = n_on;
            res[1] = n_pre;
        }
    }
    if (mbox) {
        // rv_prove's early path: what k_publish used to copy for the host in a launch of its own -- comm, the opening map, the two
        // counts (the bytes behind `comm` in device memory, in that order) -- into the host-mapped mailbox, then the stamp
        if (lane < 8) mbox[lane] = s_comm[lane];
        mbox[8 + lane] = (uint32_t)s_omit[4 * lane] | ((uint32_t)s_omit[4 * lane + 1] << 8) | ((uint32_t)s_omit[4 * lane + 2] << 16) | ((uint32_t)s_omit[4 * lane + 3] << 24);
        if (lane == 0) mbox[8 + RV_TOTAL_REPS / 4] = n_on, mbox[9 + RV_TOTAL_REPS / 4] = n_pre;
        __threadfence_system();
        __syncthreads();
        if (lane == 0) __hip_atomic_store(mbox_flag, mbox_seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
    }
}
};
__global__ __launch_bounds__(64) void k_fs_challenge(const uint8_t* __restrict__ h, FsLayout L, uint32_t rep_begin, uint32_t R, uint8_t* __restrict__ comm, uint8_t* __restrict__ omit, uint8_t* __restrict__ omit_all, uint64_t* __restrict__ offs, OnlineList* __restrict__ ol, uint32_t* __restrict__ res, uint32_t* __restrict__ mbox, uint32_t* __restrict__ mbox_flag, uint32_t mbox_seq) {
    B_k_fs_challenge{}(h, L, rep_begin, R, comm, omit, omit_all, offs, ol, res, mbox, mbox_flag, mbox_seq);
}

void launch_fs_challenge(hipStream_t st, const uint8_t* d_h, const FsLayout& L, uint32_t rep_begin, uint32_t R, uint8_t* d_comm,
                         uint8_t* d_omit, uint8_t* d_omit_all, uint64_t* d_offs, OnlineList* d_ol, uint32_t* d_res, uint32_t* mbox, uint32_t* mbox_flag,
                         uint32_t mbox_seq) {
    launch<B_k_fs_challenge, 64>(k_fs_challenge, st, dim3(1), dim3(64), d_h, L, rep_begin, R, d_comm, d_omit, d_omit_all, d_offs, d_ol, d_res, mbox, mbox_flag,
                                 mbox_seq);
}

uint32_t extract_tile_bytes(uint64_t n_items) { return ex_tb_for(n_items / 8 + 1, EXR_TB); }
uint32_t extract_from_bits_tile_bytes(uint64_t n_items) { return ex_tb_for(n_items / 8 + 1); }
void launch_extract_bits(hipStream_t st, const void* d_stream, const uint32_t* d_rows, uint64_t n_items, uint32_t NQ,
                         int kind, const uint8_t* d_omit, const uint64_t* d_dst_off, uint8_t* d_out, uint8_t* d_out2, uint32_t n_direct) {
    const uint64_t n_bytes = n_items / 8 + 1;
    const uint32_t tb = ex_tb_for(n_bytes, EXR_TB);
    const dim3 grid((unsigned)((n_bytes + tb - 1) / tb));
    if (!n_direct) d_out2 = nullptr;
    if (kind == 0)
        launch<B_k_extract_rows<0>, 256>(k_extract_rows<0>, st, grid, dim3(256), (const uint32_t*)d_stream, d_rows, n_items, NQ, tb, d_omit,
                           d_dst_off, d_out, 0, d_out2, n_direct);
    else
        launch<B_k_extract_rows<1>, 256>(k_extract_rows<1>, st, grid, dim3(256), (const uint32_t*)d_stream, d_rows, n_items, NQ, tb, d_omit,
                           d_dst_off, d_out, 0, (uint8_t*)nullptr, 0u);
}

// Inverse for the verifier (Pack::unpack / PackSelected::unpack_selected): builds dense
// rows from the proof's bit vectors.  kind 0: bit placed at the omitted player's position;
// kind 1: smeared 0x00/0xFF byte.  Reps that are not online-verified, and items beyond a
// vector's end, read as zero (verifier/online.rs:124,162,170 `unwrap_or_default`).
// A workgroup rebuilds 8*UNP_TB consecutive rows: the UNP_TB source bytes of every opened repetition are staged in
// LDS first (coalesced reads, one slot per opened repetition), then thread = (row, quad) assembles its word from LDS
// and the rows leave as full-width coalesced stores.  (One thread per word with four scattered byte loads from the
// proof took 2.0 ms per vector on the headline circuit; this takes 0.3: the 1.28 GB of rows written are the cost.)
constexpr uint32_t UNP_TB = 64;
struct B_k_unpack_bits {
    __device__ __forceinline__ void operator()(const uint8_t* __restrict__ blob, const uint64_t* __restrict__ src_off, const uint64_t* __restrict__ src_len, const uint8_t* __restrict__ omit, uint64_t n_items, uint32_t NQ, int kind, uint32_t* __restrict__ rows_out, uint32_t out_nq, uint64_t first_item) const {
    // first_item: the vectors' item the output starts at (the streaming verifier rebuilds a chunk's rows: any bit offset);
    // a slot's staged bytes are UNP_TB + 1 so that the shifted window of the last items has its second byte.  The bytes
    // arrive as ALIGNED 32-bit loads (a slot's window starts at any byte of the proof: up to 3 bytes of slack in front,
    // `s_mis`), bytes outside the vector zeroed -- bytewise loads from 40 streams made the staging the longest part
    constexpr uint32_t SB = UNP_TB + 1, SW = (SB + 3 + 3) / 4, SBP = 4 * SW;  // words / padded bytes per slot
    __shared__ __attribute__((aligned(4))) uint8_t s_bytes[RV_ONLINE_REPS * SBP];
    __shared__ uint8_t s_slot[256];
    __shared__ uint8_t s_mis[RV_ONLINE_REPS];
    __shared__ uint64_t s_off[RV_ONLINE_REPS], s_len[RV_ONLINE_REPS];
    __shared__ uint32_t s_cnt[4];
    const uint32_t R = 4 * NQ;
    const uint32_t tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    // slot of every opened repetition of the shard (rank among the opened ones; at most RV_ONLINE_REPS)
    const bool on = tid < R && omit[tid] < 8;
    const unsigned long long bal = __ballot(on);
    if (lane == 0) s_cnt[wave] = (uint32_t)__popcll(bal);
    __syncthreads();
    uint32_t base = 0;
    for (uint32_t w = 0; w < wave; w++) base += s_cnt[w];
    const uint32_t slot = base + (uint32_t)__popcll(bal & ((1ull << lane) - 1ull));
    const bool have = on && slot < RV_ONLINE_REPS;
    s_slot[tid] = have ? (uint8_t)slot : (uint8_t)0xFF;
    if (have) {
        s_off[slot] = src_off[tid];
        s_len[slot] = src_len[tid];
    }
    uint32_t n_slots = s_cnt[0] + s_cnt[1] + s_cnt[2] + s_cnt[3];
    if (n_slots > RV_ONLINE_REPS) n_slots = RV_ONLINE_REPS;
    __syncthreads();
    const uint64_t t0 = (uint64_t)blockIdx.x * UNP_TB;  // first output byte column of this workgroup
    const uint64_t b0 = first_item / 8 + t0;              // ... and the source byte it starts in
    const uint32_t sh = (uint32_t)(first_item & 7);       // output item il of the workgroup <-> source bit sh + il from byte b0
    for (uint32_t i = tid; i < n_slots * SW; i += 256) {
        const uint32_t k = i / SW, j = i % SW;
        const uint64_t len = s_len[k];
        const uintptr_t start = (uintptr_t)blob + s_off[k] + b0;  // first wanted byte; the vector ends at vend (past it: zero)
        const uintptr_t vend = (uintptr_t)blob + s_off[k] + (len < b0 + SB ? len : b0 + SB);
        const uintptr_t a = (start & ~(uintptr_t)3) + 4 * j;
        uint32_t v = 0;
        if (b0 < len && a + 4 > start && a < vend) {
            v = *(const uint32_t*)a;  // (inside the proof's allocation: it contains a byte of the vector, and the arena rounds to 256)
            const uint32_t lo = start > a ? (uint32_t)(start - a) : 0u, hi = vend < a + 4 ? (uint32_t)(vend - a) : 4u;
            const uint32_t m = (hi >= 4 ? 0xFFFFFFFFu : ((1u << (8 * hi)) - 1u)) & ~((1u << (8 * lo)) - 1u);
            v &= m;
        }
        ((uint32_t*)s_bytes)[k * SW + j] = v;
        if (j == 0) s_mis[k] = (uint8_t)(start & 3);
    }
    __syncthreads();
    const uint64_t it0 = 8 * t0;
    const uint64_t n_here = (n_items - it0 < 8ull * UNP_TB) ? n_items - it0 : 8ull * UNP_TB;
    if (256 % NQ == 0) {
        // a thread keeps its quad for the whole loop: which of its four repetitions are opened, where their bytes start in
        // LDS and the word each contributes stay in registers; only the quads that hold an opened repetition are written at
        // all -- the interpreter reads no others -- and the threads are dealt over exactly those quads (in the verifier's
        // slot order: the first ten).  A step takes one source byte column: two LDS bytes per repetition give eight items.
        __shared__ uint8_t s_quads[64];
        __shared__ uint32_t s_nq;
        if (tid < 64) {
            const bool has = tid < NQ && (s_slot[4 * tid] & s_slot[4 * tid + 1] & s_slot[4 * tid + 2] & s_slot[4 * tid + 3]) != 0xFF;
            // ... rounded to whole 32-byte sectors (eight quads; the others get zeros): a row's ten quads are a full sector and
            // a quarter of the next, and partial-sector writes cost the memory side a read-modify-write each
            const unsigned long long bh = __ballot(has);
            const bool wr = tid < NQ && ((bh >> (tid & ~7u)) & 0xFFull) != 0;
            const unsigned long long bq = __ballot(wr);
            if (wr) s_quads[__popcll(bq & ((1ull << tid) - 1ull))] = (uint8_t)tid;
            if (tid == 0) s_nq = (uint32_t)__popcll(bq);
        }
        __syncthreads();
        const uint32_t nq = s_nq;
        if (!nq || tid >= nq * (256 / nq)) return;
        const uint32_t q = s_quads[tid % nq], step = 256 / nq;
        uint32_t at[4], val[4];
#pragma unroll
        for (int i = 0; i < 4; i++) {
            const uint32_t sl = s_slot[4 * q + i];
            at[i] = sl == 0xFF ? 0xFFFFFFFFu : sl * SBP + s_mis[sl];
            val[i] = (kind == 0) ? (1u << (31u - 8u * i - (omit[4 * q + i] & 7u))) : (0xFFu << (24 - 8 * i));
        }
        for (uint32_t t = tid / nq; 8 * t < n_here; t += step) {
            uint32_t bits[4];  // item j of the column <-> bit 7 - j
#pragma unroll
            for (int i = 0; i < 4; i++) {
                bits[i] = 0;
                if (at[i] != 0xFFFFFFFFu)
                    bits[i] = ((((uint32_t)s_bytes[at[i] + t] << 8) | (uint32_t)s_bytes[at[i] + t + 1]) >> (8 - sh)) & 0xFFu;
            }
            const uint32_t nj = n_here - 8 * t < 8 ? (uint32_t)(n_here - 8 * t) : 8u;
            uint32_t* dst = rows_out + (it0 + 8 * t) * out_nq + q;
#pragma unroll
            for (uint32_t j = 0; j < 8; j++) {
                uint32_t w = 0;
#pragma unroll
                for (int i = 0; i < 4; i++) w |= ((bits[i] >> (7 - j)) & 1u) ? val[i] : 0u;
                if (j < nj) dst[(size_t)j * out_nq] = w;
            }
        }
        return;
    }
    // (odd row widths: the plain loop)
    auto src_bit = [&](uint32_t sl, uint32_t il) {
        return ((uint32_t)s_bytes[sl * SBP + s_mis[sl] + ((sh + il) >> 3)] >> (7 - ((sh + il) & 7))) & 1u;
    };
    for (uint32_t idx = tid; idx < n_here * NQ; idx += 256) {
        const uint32_t il = idx / NQ, q = idx % NQ;
        uint32_t w = 0;
#pragma unroll
        for (int i = 0; i < 4; i++) {
            const uint32_t sl = s_slot[4 * q + i];
            if (sl != 0xFF) {
                const uint32_t bit = src_bit(sl, il);
                if (bit) w |= (kind == 0) ? (1u << (31u - 8u * i - omit[4 * q + i])) : (0xFFu << (24 - 8 * i));
            }
        }
        if (q < out_nq) rows_out[(it0 + il) * out_nq + q] = w;
    }
}
};
__global__ __launch_bounds__(256) void k_unpack_bits(const uint8_t* __restrict__ blob, const uint64_t* __restrict__ src_off, const uint64_t* __restrict__ src_len, const uint8_t* __restrict__ omit, uint64_t n_items, uint32_t NQ, int kind, uint32_t* __restrict__ rows_out, uint32_t out_nq, uint64_t first_item) {
    B_k_unpack_bits{}(blob, src_off, src_len, omit, n_items, NQ, kind, rows_out, out_nq, first_item);
}

void launch_unpack_bits(hipStream_t st, const uint8_t* d_blob, const uint64_t* d_src_off, const uint64_t* d_src_len,
                        const uint8_t* d_omit, uint64_t n_items, uint32_t NQ, int kind, uint32_t* d_rows_out, uint32_t out_nq, uint64_t first_item) {
    if (!n_items) return;
    const uint64_t n_bytes = (n_items + 7) / 8;
    launch<B_k_unpack_bits, 256>(k_unpack_bits, st, dim3((unsigned)((n_bytes + UNP_TB - 1) / UNP_TB)), dim3(256), d_blob, d_src_off, d_src_len,
                                 d_omit, n_items, NQ, kind, d_rows_out, out_nq, first_item);
}

// Fixed-size parts of the openings.
//   online rep : omit | keys[8][16] with the omitted key zeroed | u64 len | .. | u64 len | .. | u64 len | ..
//   other rep  : seed[16] | H_on[32]                           (proof/mod.rs:41-53, prover.rs:125-136,167-170)
// d_off2/d_off64 give each rep's record offset inside the shard's concatenated output.
struct B_k_open_headers {
    // workgroup = (repetition, domain), thread = one header byte (consecutive lanes write consecutive bytes: the stores
    // coalesce, also when the proof buffer is mapped host memory); a lane-per-repetition version that walked its ~300
    // bytes one by one took 14 us of a 0.5 ms AES-128 proof
    __device__ __forceinline__ void operator()(uint32_t R, const uint8_t* __restrict__ omit, const uint8_t* __restrict__ seeds, const uint8_t* __restrict__ keys, const uint32_t* __restrict__ on2, const uint32_t* __restrict__ on64, const uint64_t* __restrict__ off2, const uint64_t* __restrict__ off64, uint64_t l2r, uint64_t l2c, uint64_t l2i, uint64_t l64r, uint64_t l64c, uint64_t l64i, uint8_t* __restrict__ out) const {
    run(blockIdx.x, R, omit, seeds, keys, on2, on64, off2, off64, l2r, l2c, l2i, l64r, l64c, l64i, out);
    }
    static __device__ __forceinline__ void run(uint32_t bx, uint32_t R, const uint8_t* __restrict__ omit, const uint8_t* __restrict__ seeds, const uint8_t* __restrict__ keys, const uint32_t* __restrict__ on2, const uint32_t* __restrict__ on64, const uint64_t* __restrict__ off2, const uint64_t* __restrict__ off64, uint64_t l2r, uint64_t l2c, uint64_t l2i, uint64_t l64r, uint64_t l64c, uint64_t l64i, uint8_t* __restrict__ out) {
    const uint32_t r = bx >> 1, dom = bx & 1u, i = threadIdx.x;
    if (r >= R) return;
    const uint32_t om = omit[r];
    uint8_t* o = out + (dom == 0 ? off2[r] : off64[r]);
    if (om < 8) {
        const uint64_t lr = dom == 0 ? l2r : l64r, lc = dom == 0 ? l2c : l64c, li = dom == 0 ? l2i : l64i;
        if (i == 0) {
            o[0] = (uint8_t)om;
        } else if (i < 129) {
            const uint32_t p = (i - 1) >> 4;
            o[i] = (p == om) ? (uint8_t)0 : keys[(size_t)r * 128 + (i - 1)];
        } else if (i < 137) {
            o[i] = (uint8_t)(lr >> (8 * (i - 129)));
        } else if (i < 145) {
            o[137 + lr + (i - 137)] = (uint8_t)(lc >> (8 * (i - 137)));
        } else if (i < 153) {
            o[145 + lr + lc + (i - 145)] = (uint8_t)(li >> (8 * (i - 145)));
        }
    } else {
        if (i < 16) {
            o[i] = seeds[(size_t)r * 16 + i];
        } else if (i < 48) {
            const uint32_t* hon = (dom == 0 ? on2 : on64) + (size_t)r * 8;
            o[i] = (uint8_t)(hon[(i - 16) >> 2] >> (8 * ((i - 16) & 3)));
        }
    }
}
};
__global__ void k_open_headers(uint32_t R, const uint8_t* __restrict__ omit, const uint8_t* __restrict__ seeds, const uint8_t* __restrict__ keys, const uint32_t* __restrict__ on2, const uint32_t* __restrict__ on64, const uint64_t* __restrict__ off2, const uint64_t* __restrict__ off64, uint64_t l2r, uint64_t l2c, uint64_t l2i, uint64_t l64r, uint64_t l64c, uint64_t l64i, uint8_t* __restrict__ out) {
    B_k_open_headers{}(R, omit, seeds, keys, on2, on64, off2, off64, l2r, l2c, l2i, l64r, l64c, l64i, out);
}

void launch_open_headers(hipStream_t st, uint32_t R, const uint8_t* d_omit, const uint8_t* d_seeds, const uint8_t* d_keys,
                         const uint32_t* d_on2, const uint32_t* d_on64, const uint64_t* d_off2, const uint64_t* d_off64,
                         uint64_t l2r, uint64_t l2c, uint64_t l2i, uint64_t l64r, uint64_t l64c, uint64_t l64i, uint8_t* d_out) {
    launch<B_k_open_headers, 192>(k_open_headers, st, dim3(2 * R), dim3(192), R, d_omit, d_seeds, d_keys, d_on2, d_on64, d_off2,
                       d_off64, l2r, l2c, l2i, l64r, l64c, l64i, d_out);
}

// ONE small GF(2) proof's openings in one launch: the record heads, the broadcast vectors, the corrections vectors and the input vectors
// are four independent pieces of work behind the challenge, each a kernel of 5 - 11 us that occupies a corner of the chip -- as ranges
// of one grid they cost one launch (and the error word for the host rides along).  Large proofs keep the separate launches: the
// pieces' LDS adds up here (58 KB per workgroup).
struct OpenSmall {
    // heads
    uint32_t R;
    const uint8_t *omit, *seeds, *keys;
    const uint32_t *on2, *on64;
    const uint64_t *off2, *off64;
    uint64_t l2r, l2c, l2i, l64r, l64c, l64i;
    // vectors
    const uint32_t *on, *rec_rows, *in_rows;
    const uint8_t* pre;
    uint64_t n_rec, n_pre, n_in;
    uint32_t NQ, tb_rec, tb_pre, tb_in;
    const uint64_t *dst_rec, *dst_in;
    const OnlineList* ol;
    uint32_t corr_rep_min;
    uint32_t g_hdr, g_rec, g_pre;  // workgroups of the first three ranges
    uint8_t* out;
    const int* err_src;
    int* err_dst;  // (nullable) host-mapped
};
__global__ __launch_bounds__(256) void k_open_small(OpenSmall a) {
    const uint32_t bx = blockIdx.x;
    if (bx < a.g_hdr) {
        if (threadIdx.x < 192) B_k_open_headers::run(bx, a.R, a.omit, a.seeds, a.keys, a.on2, a.on64, a.off2, a.off64, a.l2r, a.l2c, a.l2i, a.l64r, a.l64c, a.l64i, a.out);
        if (bx == 0 && threadIdx.x == 255 && a.err_dst) *a.err_dst = *a.err_src;
    } else if (bx < a.g_hdr + a.g_rec) {
        B_k_extract_rows<0>{}(a.on, a.rec_rows, a.n_rec, a.NQ, a.tb_rec, a.omit, a.dst_rec, a.out, 0u - a.g_hdr);
    } else if (bx < a.g_hdr + a.g_rec + a.g_pre) {
        B_k_extract_from_bits{}(a.pre, a.n_pre, a.NQ, a.tb_pre, a.ol, a.out, a.corr_rep_min, 0u - (a.g_hdr + a.g_rec));
    } else {
        B_k_extract_rows<1>{}(a.on, a.in_rows, a.n_in, a.NQ, a.tb_in, a.omit, a.dst_in, a.out, 0u - (a.g_hdr + a.g_rec + a.g_pre));
    }
}
// true (and the launch made) when the proof is small enough and nothing records launches; otherwise the caller launches the pieces
// heads_inputs_only: the record heads and the input vectors only (a large proof: its broadcast and corrections vectors keep their launches)
bool launch_open_small(hipStream_t st, uint32_t R, const uint8_t* d_omit, const uint8_t* d_seeds, const uint8_t* d_keys, const uint32_t* d_on2,
                       const uint32_t* d_on64, const uint64_t* d_offs /* [8][R] as shard_open_impl lays them out */, uint64_t l2r, uint64_t l2c, uint64_t l2i,
                       uint64_t l64r, uint64_t l64c, uint64_t l64i, const uint32_t* d_on, const uint32_t* d_rec_rows, uint64_t n_rec, const uint8_t* d_pre,
                       uint64_t n_pre, const uint32_t* d_in_rows, uint64_t n_in, uint32_t NQ, const OnlineList* d_ol, uint32_t corr_rep_min, uint8_t* d_out,
                       const int* d_err, int* err_dst_mapped, bool heads_inputs_only) {
    if (g_recorder) return false;
    OpenSmall a{};
    a.tb_rec = ex_tb_for(n_rec / 8 + 1, EXR_TB), a.tb_pre = ex_tb_for(n_pre / 8 + 1), a.tb_in = ex_tb_for(n_in / 8 + 1, EXR_TB);
    a.g_hdr = 2 * R;
    a.g_rec = heads_inputs_only ? 0u : (uint32_t)((n_rec / 8 + 1 + a.tb_rec - 1) / a.tb_rec);
    a.g_pre = !heads_inputs_only && corr_rep_min < R ? (uint32_t)((n_pre / 8 + 1 + a.tb_pre - 1) / a.tb_pre) : 0u;
    const uint32_t g_in = (uint32_t)((n_in / 8 + 1 + a.tb_in - 1) / a.tb_in);
    // (the sizes at which a launch matters: vectors of a few KB.  Longer ones keep their own launches -- 58 KB of LDS per workgroup here
    // against 20 there: the 10^7-gate circuit's openings took 470 us this way instead of 360)
    if ((uint64_t)a.g_rec + a.g_pre + g_in > 2048) return false;
    a.R = R, a.omit = d_omit, a.seeds = d_seeds, a.keys = d_keys, a.on2 = d_on2, a.on64 = d_on64, a.off2 = d_offs, a.off64 = d_offs + R;
    a.l2r = l2r, a.l2c = l2c, a.l2i = l2i, a.l64r = l64r, a.l64c = l64c, a.l64i = l64i;
    a.on = d_on, a.rec_rows = d_rec_rows, a.in_rows = d_in_rows, a.pre = d_pre, a.n_rec = n_rec, a.n_pre = n_pre, a.n_in = n_in, a.NQ = NQ;
    a.dst_rec = d_offs + 2 * (size_t)R, a.dst_in = d_offs + 4 * (size_t)R, a.ol = d_ol, a.corr_rep_min = corr_rep_min;
    a.out = d_out, a.err_src = d_err, a.err_dst = err_dst_mapped;
    hipLaunchKernelGGL(k_open_small, dim3(a.g_hdr + a.g_rec + a.g_pre + g_in), dim3(256), 0, st, a);
    return true;
}

// the device error word into a host-mapped word (small proofs leave without a copy engine: api.hip, rv_prove_impl)
__global__ void k_store_word(const int* __restrict__ src, int* __restrict__ dst) { *dst = *src; }
void launch_store_word(hipStream_t st, const int* d_src, int* dst_mapped) { hipLaunchKernelGGL(k_store_word, dim3(1), dim3(1), 0, st, d_src, dst_mapped); }
// a few KB (the verifier's 256 digests) plus the error word into host-mapped memory, for the same reason
__global__ void k_store_words(const uint32_t* __restrict__ src, uint32_t n_words, uint32_t* __restrict__ dst, const int* __restrict__ err, int* __restrict__ dst_err) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n_words) dst[i] = src[i];
    if (i == 0 && err) *dst_err = *err;
}
void launch_store_words(hipStream_t st, const uint32_t* d_src, uint32_t n_words, uint32_t* dst_mapped, const int* d_err, int* dst_err_mapped) {
    hipLaunchKernelGGL(k_store_words, dim3((n_words + 255) / 256), dim3(256), 0, st, d_src, n_words, dst_mapped, d_err, dst_err_mapped);
}
// The four repetition counts of bincode(Proof) -- 40, 216, 40, 216, u64 little-endian in front of their sections -- for `batch`
// framed proofs that lie `stride` bytes apart (rv_prove_batch_device: the host form patches them into its copy).  One thread per
// count; the offsets are multiples of 8 (a section is 40 records or 216 x 48 bytes) and the proofs 256-byte aligned.
struct FrameCounts {
    uint64_t off[4], value[4];
};
__global__ __launch_bounds__(256) void k_frame_counts(uint8_t* __restrict__ out, uint64_t stride, uint32_t batch, FrameCounts f) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= batch * 4u) return;
    const uint32_t b = i >> 2, k = i & 3u;
    *(uint64_t*)(out + (size_t)b * stride + f.off[k]) = f.value[k];
}
bool launch_frame_counts(hipStream_t st, uint8_t* d_out, uint64_t stride, uint32_t batch, const size_t lens[4]) {
    FrameCounts f{};
    uint64_t off = 32;
    for (int k = 0; k < 4; k++) {
        f.off[k] = off;
        f.value[k] = k % 2 ? RV_PREPROCESSING_REPS : RV_ONLINE_REPS;
        off += 8 + lens[k];
    }
    if (!batch || batch > 0x3FFFFFFFu || (((uintptr_t)d_out | stride | f.off[0] | f.off[1] | f.off[2] | f.off[3]) & 7)) return false;
    hipLaunchKernelGGL(k_frame_counts, dim3((batch * 4 + 255) / 256), dim3(256), 0, st, d_out, stride, batch, f);
    return true;
}

// ------------------------------------------------------------------------------------
// Early corrections (api.hip, rv_prove on large GF(2) circuits).  The corrections vector of an opened repetition
// (Pack of ReconGF2, gf2/recon.rs:189-239: one bit per Mul, 8 per byte MSB-first, n/8 + 1 bytes) depends on the
// challenge only through WHICH repetitions open, and it is half of the proof.  So the packed vector of EVERY repetition
// is produced while the interpreter still runs -- a range of the preprocessing rows at a time, as soon as the levels that
// write them are done -- and leaves for the host through the copy engine before the challenge exists; after the
// challenge the host copies the 40 it needs into the proof and only the other half crosses PCIe behind the last kernel.
//
// k_pack_corr_all: workgroup = PC_TB output bytes (8 * PC_TB rows of 32 bytes, contiguous) of all 256 repetitions.
// A thread takes eight consecutive rows x four byte columns at a time: eight 32-bit loads, byte transposes (v_perm) into
// four words pairs with a row per byte, and for each column the 8 x 8 bit transpose of Hacker's Delight (transpose8rS32)
// -- eight output bytes, one per repetition of the column's byte, for ~5 instructions each (a lane per repetition
// picking one bit out of each of its eight rows took 14 and two quarter-rate multiplications).  The bytes are collected
// per repetition in LDS and written out as runs of two whole sectors (PC_TB = 64 bytes per workgroup and repetition; 128: 27 instead
// of 24.5 us per 27 MB chunk -- twice the workgroups in flight).
// out: [256][pitch], pitch a multiple of 128; byte0 = first byte of the chunk within a repetition's vector.
// ------------------------------------------------------------------------------------
constexpr uint32_t PC_TB = 64;
constexpr uint32_t PC_OSTRIDE = PC_TB + 4;  // bytes per repetition in the LDS output tile: 33 dwords
__global__ __launch_bounds__(256) void k_pack_corr_all(const uint8_t* __restrict__ bits /*[n_items][32]*/, uint64_t n_items, uint64_t byte0,
                                                       uint64_t n_bytes, uint64_t pitch, uint8_t* __restrict__ out) {
    __shared__ __attribute__((aligned(16))) uint8_t s_out[256 * PC_OSTRIDE];
    const uint64_t t0 = (uint64_t)blockIdx.x * PC_TB;
    const uint32_t nb = (uint32_t)((n_bytes - t0 < PC_TB) ? n_bytes - t0 : PC_TB);
    const uint64_t r0 = 8 * (byte0 + t0);
    const uint32_t n_rows = (uint32_t)(r0 >= n_items ? 0 : (n_items - r0 < 8ull * nb ? n_items - r0 : 8ull * nb));  // rows past the end are zero bits
    const uint8_t* src = bits + r0 * 32;
    // item = (output byte tl, column quad cq): rows 8 tl .. 8 tl + 7, byte columns 4 cq .. 4 cq + 3; a wavefront's 64 items
    // cover 64 consecutive rows.  All of a thread's 32 loads are issued before the first transpose.
    constexpr int ITEMS = PC_TB * 8 / 256;
    uint32_t w[ITEMS][8];
#pragma unroll
    for (int n = 0; n < ITEMS; n++) {
        const uint32_t it = threadIdx.x + 256 * n, cq = it & 7, tl = it >> 3;
#pragma unroll
        for (int j = 0; j < 8; j++) w[n][j] = (8 * tl + j < n_rows) ? *(const uint32_t*)(src + (size_t)(8 * tl + j) * 32 + 4 * cq) : 0u;
    }
#pragma unroll
    for (int n = 0; n < ITEMS; n++) {
        const uint32_t it = threadIdx.x + 256 * n, cq = it & 7, tl = it >> 3;
        if (tl >= nb) continue;
        // xs[k] = rows 0..3 of column 4 cq + k, row 0 in the top byte; ys[k] = rows 4..7
        uint32_t xs[4], ys[4];
        {
            const uint32_t a = __builtin_amdgcn_perm(w[n][2], w[n][3], 0x05010400u), b = __builtin_amdgcn_perm(w[n][2], w[n][3], 0x07030602u);
            const uint32_t c = __builtin_amdgcn_perm(w[n][0], w[n][1], 0x05010400u), d = __builtin_amdgcn_perm(w[n][0], w[n][1], 0x07030602u);
            xs[0] = __builtin_amdgcn_perm(c, a, 0x05040100u), xs[1] = __builtin_amdgcn_perm(c, a, 0x07060302u);
            xs[2] = __builtin_amdgcn_perm(d, b, 0x05040100u), xs[3] = __builtin_amdgcn_perm(d, b, 0x07060302u);
        }
        {
            const uint32_t a = __builtin_amdgcn_perm(w[n][6], w[n][7], 0x05010400u), b = __builtin_amdgcn_perm(w[n][6], w[n][7], 0x07030602u);
            const uint32_t c = __builtin_amdgcn_perm(w[n][4], w[n][5], 0x05010400u), d = __builtin_amdgcn_perm(w[n][4], w[n][5], 0x07030602u);
            ys[0] = __builtin_amdgcn_perm(c, a, 0x05040100u), ys[1] = __builtin_amdgcn_perm(c, a, 0x07060302u);
            ys[2] = __builtin_amdgcn_perm(d, b, 0x05040100u), ys[3] = __builtin_amdgcn_perm(d, b, 0x07060302u);
        }
#pragma unroll
        for (int k = 0; k < 4; k++) {
            uint32_t x = xs[k], y = ys[k], t;
            t = (x ^ (x >> 7)) & 0x00AA00AAu, x = x ^ t ^ (t << 7);
            t = (y ^ (y >> 7)) & 0x00AA00AAu, y = y ^ t ^ (t << 7);
            t = (x ^ (x >> 14)) & 0x0000CCCCu, x = x ^ t ^ (t << 14);
            t = (y ^ (y >> 14)) & 0x0000CCCCu, y = y ^ t ^ (t << 14);
            t = (x & 0xF0F0F0F0u) | ((y >> 4) & 0x0F0F0F0Fu);
            y = ((x << 4) & 0xF0F0F0F0u) | (y & 0x0F0F0F0Fu);
            x = t;
            // byte i of (x, y) from the top = input bit 7 - i of every row, row j at output bit 7 - j.  Nibble bit p of a byte
            // <-> repetition 8 c + 3 - p (p < 4), 8 c + 11 - p (p >= 4), as k_extract_from_bits: x = repetitions 8 c + 4 .. + 7, y = 8 c .. + 3
            uint8_t* o = s_out + (size_t)(8 * (4 * cq + k)) * PC_OSTRIDE + tl;
            o[4 * PC_OSTRIDE] = (uint8_t)(x >> 24), o[5 * PC_OSTRIDE] = (uint8_t)(x >> 16), o[6 * PC_OSTRIDE] = (uint8_t)(x >> 8), o[7 * PC_OSTRIDE] = (uint8_t)x;
            o[0 * PC_OSTRIDE] = (uint8_t)(y >> 24), o[1 * PC_OSTRIDE] = (uint8_t)(y >> 16), o[2 * PC_OSTRIDE] = (uint8_t)(y >> 8), o[3 * PC_OSTRIDE] = (uint8_t)y;
        }
    }
    __syncthreads();
    // 16 bytes per thread and step, PC_TB / 16 threads per repetition: whole sectors
    for (uint32_t i = threadIdx.x; i < 256 * (PC_TB / 16); i += 256) {
        const uint32_t r = i / (PC_TB / 16), k = i % (PC_TB / 16);
        if (16 * k < nb) {  // (the bytes past nb inside the last 16 are pitch padding)
            const uint32_t* sp = (const uint32_t*)(s_out + r * PC_OSTRIDE + 16 * k);
            *(uint4*)(out + (size_t)r * pitch + t0 + 16 * k) = make_uint4(sp[0], sp[1], sp[2], sp[3]);
        }
    }
}
void launch_pack_corr_all(hipStream_t st, const uint8_t* d_bits, uint64_t n_items, uint64_t byte0, uint64_t n_bytes, uint64_t pitch, uint8_t* d_out) {
    if (!n_bytes) return;
    hipLaunchKernelGGL(k_pack_corr_all, dim3((unsigned)((n_bytes + PC_TB - 1) / PC_TB)), dim3(256), 0, st, d_bits, n_items, byte0, n_bytes, pitch, d_out);
}

// The proof image in HBM to the page-locked proof buffer WITHOUT the corrections vectors of its first m online records, m =
// the opened repetitions below rep_limit (omit[r] < 8; all n_rec of them when rep_limit = 256).  Record j: image bytes
// [first + j * rec, ...), its corrections at [+ corr_at, + corr_at + corr_len).  Piece j (blockIdx.y) runs from the end of record
// j - 1's corrections to the start of record j's, piece m to the end of the image.  Source and destination offsets are equal,
// both bases 16-byte aligned.
__global__ __launch_bounds__(256) void k_copy_gaps(const uint8_t* __restrict__ img, uint8_t* __restrict__ dst_mapped, uint64_t total, uint64_t first,
                                                   uint64_t rec, uint64_t corr_at, uint64_t corr_len, uint32_t n_rec, const uint8_t* __restrict__ omit,
                                                   uint32_t rep_limit, OpenDirect od, const int* __restrict__ err_src, int* __restrict__ err_dst) {
    __shared__ uint32_t s_m;
    if (err_dst && blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x == 255) *err_dst = *err_src;  // (the error word for the host rides along)
    if (threadIdx.x < 64) {
        uint32_t cnt = 0;
        for (uint32_t r = threadIdx.x; r < rep_limit && r < RV_TOTAL_REPS; r += 64) cnt += omit[r] < 8 ? 1u : 0u;
        for (int o = 32; o; o >>= 1) cnt += __shfl_xor(cnt, o);
        if (threadIdx.x == 0) s_m = cnt < n_rec ? cnt : n_rec;
    }
    __syncthreads();
    const uint32_t m = s_m, j = blockIdx.y;
    if (j > m) return;
    const uint64_t a = j == 0 ? 0 : first + (uint64_t)(j - 1) * rec + corr_at + corr_len;
    const uint64_t b = j == m ? total : first + (uint64_t)j * rec + corr_at;
    if (b <= a) return;
    uint64_t a16 = (a + 15) & ~15ull, b16 = b & ~15ull;
    if (a16 > b16) a16 = b16 = b;  // shorter than one aligned word: bytes only
    const uint64_t tid = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x, nth = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t i = a + tid; i < a16; i += nth) dst_mapped[i] = img[i];
    if (od.n_direct && j < m) {
        // record j's broadcast vector lies in this piece: the words inside the tiles the extraction kernel has sent already are left
        // out (the image holds every tile, so a word across the boundary is simply copied)
        const uint64_t v0 = first + (uint64_t)j * rec + od.rvec_at;
        const uint64_t v1 = std::min(v0 + (uint64_t)od.n_direct * od.tile, v0 + od.rvec_len);  // [v0, v1): the tiles sent already
        const uint64_t ve = v0 + od.rvec_len;
        for (uint64_t i = a16 + 16 * tid; i < b16; i += 16 * nth) {
            // a whole word of the vector that starts in one of those tiles is there (k_extract_rows: LA)
            if (i >= v0 && i < v1 && i + 16 <= ve) {
                const uint64_t last = std::min(v1, ve - 15);                        // first word start that is NOT there (or beyond)
                const uint64_t nsk = (last - i + 16 * nth - 1) / (16 * nth);  // this thread's words up to it
                i += (nsk - 1) * 16 * nth;
                continue;
            }
            *(uint4*)(dst_mapped + i) = *(const uint4*)(img + i);
        }
    } else {
        for (uint64_t i = a16 + 16 * tid; i < b16; i += 16 * nth) *(uint4*)(dst_mapped + i) = *(const uint4*)(img + i);
    }
    for (uint64_t i = b16 + tid; i < b; i += nth) dst_mapped[i] = img[i];
}
void launch_copy_gaps(hipStream_t st, const uint8_t* d_img, uint8_t* dst_mapped, uint64_t total, uint64_t first, uint64_t rec, uint64_t corr_at,
                      uint64_t corr_len, uint32_t n_rec, const uint8_t* d_omit, uint32_t rep_limit, OpenDirect od, const int* d_err, int* err_dst_mapped) {
    if (!od.n_direct || od.tile < 16 || (od.tile & (od.tile - 1))) od = OpenDirect();
    // (the last piece may be most of the image -- Z64 with few staged repetitions --: enough workgroups per piece to fill PCIe alone)
    hipLaunchKernelGGL(k_copy_gaps, dim3(rep_limit < RV_TOTAL_REPS ? 64 : 8, n_rec + 1), dim3(256), 0, st, d_img, dst_mapped, total, first, rec, corr_at, corr_len,
                       n_rec, d_omit, rep_limit, od, d_err, err_dst_mapped);
}

// n_words of device memory into host-mapped memory, then (ordered behind them at system scope) a sequence number the
// host polls: how the host learns the challenge in the middle of a proof without a stream synchronisation
__global__ __launch_bounds__(256) void k_publish(const uint32_t* __restrict__ src, uint32_t n_words, uint32_t* __restrict__ dst_mapped, uint32_t* __restrict__ flag_mapped, uint32_t seq) {
    for (uint32_t i = threadIdx.x; i < n_words; i += blockDim.x) dst_mapped[i] = src[i];  // (n_words = 0: a progress stamp only)
    __threadfence_system();
    __syncthreads();
    if (threadIdx.x == 0) __hip_atomic_store(flag_mapped, seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
}
void launch_publish(hipStream_t st, const uint32_t* d_src, uint32_t n_words, uint32_t* dst_mapped, uint32_t* flag_mapped, uint32_t seq) {
    hipLaunchKernelGGL(k_publish, dim3(1), dim3(n_words ? 256 : 64), 0, st, d_src, n_words, dst_mapped, flag_mapped, seq);
}

}  // namespace rv
