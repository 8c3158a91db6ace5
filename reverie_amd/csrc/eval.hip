// Cleartext evaluation (rv_evaluate / rv_evaluate_batch / rv_evaluate_batch_device, host side in eval.inc): the compiled gate stream run on witness values
// alone -- no shares, no masks, no transcripts -- for many witnesses at once.
//
// Values, one set per witness b of the batch:
//   GF(2): val[row][W] u32, W = ceil(B / 32): bit b % 32 of word b / 32 of a row is witness b's value of that share row (rows are the
//          compiled gates' row ids, the index space of InterpParams::vclr); the zero row holds zeros.
//   Z64:   v64[ssa][B] u64; SSA id 0 (the never-written wire) holds zeros.
// Per gate the MODE_PROVE_V branches of k_interp_full (interp.hip): Input copies the witness bit, Xor sums its base rows, Mul ANDs
// its two operand forms, AssertZero records the witnesses whose operand is not zero.  B2A (combine.rs:132-219) is compiled into 64
// fresh GF(2) masks, a ripple-carry adder and 64 revealed sum bits: with every fresh mask taken as zero (G_RANDOM writes zeros --
// the op list has no Random op of its own, the caller checked) the sum bits ARE the source bits, and the Z64 value is their binary
// number.
#include "internal.h"

namespace rv {

namespace {

// value of the XOR of n base rows, word j
// (no __restrict__ on the value arrays: the walking kernel reads, level after level, what its own threads wrote)
__device__ __forceinline__ uint32_t ev_sum(const uint32_t* val, const uint32_t* ids, uint32_t n, uint32_t W, uint32_t j) {
    uint32_t v = 0;
    for (uint32_t i = 0; i < n; i++) v ^= val[(size_t)ids[i] * W + j];
    return v;
}

// a failing AssertZero: every witness whose bit is set counts it, and the first one in program order (smallest reconstruction ordinal
// of its domain) is kept.  Failures are rare: an atomic per failing witness.
__device__ __forceinline__ void ev_fail(const EvalParams& p, uint32_t b, uint32_t x, uint32_t* first) {
    atomicAdd(&p.n_failed[b], 1u);
    atomicMin(&first[b], x);
}

__device__ __forceinline__ void ev_gf2(const EvalParams& p, const Gate& g, uint32_t j) {
    const uint32_t W = p.W;
    uint32_t* val = p.val;
    switch (g_op(g)) {
    case G_INPUT:
        val[(size_t)g.dst * W + j] = p.win[(size_t)g.x * W + j];
        break;
    case G_XORK:
        val[(size_t)g.dst * W + j] = ev_sum(val, g.a, g_na(g), W, j) ^ ev_sum(val, g.b, g_nb(g), W, j) ^ (g_ca(g) ? ~0u : 0u);
        break;
    case G_MUL: {
        const uint32_t x = ev_sum(val, g.a, g_na(g), W, j) ^ (g_ca(g) ? ~0u : 0u);
        const uint32_t y = ev_sum(val, g.b, g_nb(g), W, j) ^ (g_cb(g) ? ~0u : 0u);
        val[(size_t)g.dst * W + j] = x & y;
        break;
    }
    case G_RANDOM:  // B2A's fresh masks (see the top of the file)
        val[(size_t)g.dst * W + j] = 0;
        break;
    case G_RECON:  // B2A's revealed sum bit: the value itself
        val[(size_t)g.dst * W + j] = ev_sum(val, g.a, g_na(g), W, j) ^ (g_ca(g) ? ~0u : 0u);
        break;
    case G_ASSERT: {
        uint32_t f = ev_sum(val, g.a, g_na(g), W, j) ^ (g_ca(g) ? ~0u : 0u);
        const uint32_t b0 = 32 * j;
        if (p.B - b0 < 32) f &= (1u << (p.B - b0)) - 1;  // (the padding lanes of the last word are no witnesses)
        while (f) {
            const uint32_t k = (uint32_t)__builtin_ctz(f);
            f &= f - 1;
            ev_fail(p, b0 + k, g.x, p.first2);
        }
        break;
    }
    }
}

__device__ __forceinline__ void ev_z64(const EvalParams& p, const Gate64& g, uint32_t b) {
    const size_t B = p.B;
    uint64_t* v = p.v64;
    // (operand a of B2A is a GF(2) row: only the Z64 gates that read Z64 operands load them)
    auto x = [&]() { return v[(size_t)g.a * B + b]; };
    auto y = [&]() { return v[(size_t)g.b * B + b]; };
    uint64_t r;
    switch (g.op) {
    case G64_INPUT: r = p.wz[(size_t)b * p.wz_stride + g.x]; break;
    case G64_ADD: r = x() + y(); break;
    case G64_SUB: r = x() - y(); break;
    case G64_ADDC: r = x() + g.imm; break;
    case G64_SUBC: r = x() - g.imm; break;
    case G64_MULC: r = x() * g.imm; break;
    case G64_MUL: r = x() * y(); break;
    case G64_CONST: r = g.imm; break;
    case G64_B2A: {
        // g.a: the first of the 64 consecutive rows of the revealed sum bits
        r = 0;
        const uint32_t j = b >> 5, sh = b & 31;
        for (uint32_t k = 0; k < 64; k++) r |= (uint64_t)((p.val[(size_t)(g.a + k) * p.W + j] >> sh) & 1u) << k;
        break;
    }
    case G64_ASSERT:
        if (x()) ev_fail(p, b, g.x, p.first64);
        return;
    default:  // G64_RANDOM: the caller refuses op lists with Random ops
        return;
    }
    v[(size_t)g.dst * B + b] = r;
}

// schedule (a): one level; threads [0, n2 * W) take (GF(2) gate, word) pairs, the rest (Z64 gate, witness) pairs
__global__ __launch_bounds__(256) void k_eval_level(EvalParams p, const Gate* __restrict__ gates, uint32_t lo, uint32_t n2,
                                                    const Gate64* __restrict__ gates64, uint32_t lo64, uint32_t n64) {
    const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const uint64_t t2 = (uint64_t)n2 * p.W;
    if (t < t2) {
        ev_gf2(p, gates[lo + t / p.W], (uint32_t)(t % p.W));
    } else if (t - t2 < (uint64_t)n64 * p.B) {
        const uint64_t u = t - t2;
        ev_z64(p, gates64[lo64 + u / p.B], (uint32_t)(u % p.B));
    }
}

// schedule (b): workgroup k owns witness words [k * S, k * S + S) (and their witnesses) and walks every level, __syncthreads() between
// two levels.  No workgroup reads what another one writes, and the waves of one workgroup share the compute unit's L1: plain accesses.
__global__ __launch_bounds__(1024) void k_eval_walk(EvalParams p, const Gate* __restrict__ gates, const LevelRange* __restrict__ lr,
                                                    const Gate64* __restrict__ gates64, const uint32_t* __restrict__ ls64, uint32_t n_levels,
                                                    uint32_t S) {
    const uint32_t j0 = blockIdx.x * S;
    const uint32_t sw = min(S, p.W - j0);
    const uint32_t b0 = 32 * j0, nb = min(p.B - b0, 32 * sw);
    for (uint32_t l = 0; l < n_levels; l++) {
        const uint32_t lo = lr[l].lo, n2 = (lr[l].hi - lo) * sw;
        for (uint32_t t = threadIdx.x; t < n2; t += blockDim.x) ev_gf2(p, gates[lo + t / sw], j0 + t % sw);
        if (ls64) {
            const uint32_t lo64 = ls64[l], n64 = (ls64[l + 1] - lo64) * nb;
            for (uint32_t t = threadIdx.x; t < n64; t += blockDim.x) ev_z64(p, gates64[lo64 + t / nb], b0 + t % nb);
        }
        __syncthreads();
    }
}

// witness bytes (0 / non-zero), witness b's n inputs at wit + b * stride -> bit-sliced input words [n][W].  One thread per output
// word, threads along the input index: the 32 byte reads of a word go down 32 witness rows, and neighbouring threads read neighbouring
// bytes of each row (a wavefront's load is 64 consecutive bytes, whatever the stride)
__global__ __launch_bounds__(256) void k_eval_wit(const uint8_t* __restrict__ wit, size_t stride, uint32_t n, uint32_t B, uint32_t W,
                                                  uint32_t* __restrict__ out) {
    const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= (uint64_t)n * W) return;
    const uint32_t i = (uint32_t)(t % n), j = (uint32_t)(t / n);
    uint32_t w = 0;
    for (uint32_t k = 0; k < 32 && 32 * j + k < B; k++) w |= (wit[(size_t)(32 * j + k) * stride + i] ? 1u : 0u) << k;
    out[(size_t)i * W + j] = w;
}

// the wires' final values -> [B][gf2_wires] bytes and [B][z64_wires] words
__global__ __launch_bounds__(256) void k_eval_out(EvalParams p, const WireForm* __restrict__ forms, uint32_t n_gf2, const uint32_t* __restrict__ ssa64,
                                                  uint32_t n_z64, uint8_t* __restrict__ out2, uint64_t* __restrict__ out64) {
    const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const uint64_t t2 = out2 ? (uint64_t)n_gf2 * p.B : 0;
    if (t < t2) {
        const uint32_t b = (uint32_t)(t / n_gf2), w = (uint32_t)(t % n_gf2);
        const WireForm f = forms[w];
        const uint32_t j = b >> 5;
        uint32_t v = f.c;
        for (int i = 0; i < RV_LIN_K; i++) v ^= p.val[(size_t)f.b[i] * p.W + j] >> (b & 31);
        out2[t] = (uint8_t)(v & 1u);
    } else if (out64 && t - t2 < (uint64_t)n_z64 * p.B) {
        const uint64_t u = t - t2;
        const uint32_t b = (uint32_t)(u / n_z64), w = (uint32_t)(u % n_z64);
        out64[u] = p.v64[(size_t)ssa64[w] * p.B + b];
    }
}

// the op-list index of the AssertZero with reconstruction ordinal x: binary search in the chunk's ordinal table (UINT64_MAX: none)
__device__ __forceinline__ uint64_t ev_assert_op(const uint32_t* rec, const uint64_t* op, uint32_t n, uint32_t x) {
    if (x == UINT32_MAX) return UINT64_MAX;
    uint32_t lo = 0, hi = n;
    while (lo < hi) {
        const uint32_t mid = lo + (hi - lo) / 2;
        if (rec[mid] < x)
            lo = mid + 1;
        else
            hi = mid;
    }
    return (lo < n && rec[lo] == x) ? op[lo] : UINT64_MAX;
}

// rv_evaluate_batch_device: the selected wires' final values of the part's witnesses -> [B][n_sel2] bytes and [B][n_sel64] words in
// the caller's buffers (out2 / out64: where the part's first witness goes; null: not wanted).  sel2 / sel64 null: wire i itself
// (every wire, in order).  Threads run along the selection index within a witness.
__global__ __launch_bounds__(256) void k_eval_out_sel(EvalParams p, const WireForm* __restrict__ forms, const uint32_t* __restrict__ sel2,
                                                      uint32_t n_sel2, const uint32_t* __restrict__ ssa64, const uint32_t* __restrict__ sel64,
                                                      uint32_t n_sel64, uint8_t* __restrict__ out2, uint64_t* __restrict__ out64) {
    const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const uint64_t t2 = out2 ? (uint64_t)n_sel2 * p.B : 0;
    if (t < t2) {
        const uint32_t b = (uint32_t)(t / n_sel2), i = (uint32_t)(t % n_sel2);
        const WireForm f = forms[sel2 ? sel2[i] : i];
        const uint32_t j = b >> 5;
        uint32_t v = f.c;
        for (int k = 0; k < RV_LIN_K; k++) v ^= p.val[(size_t)f.b[k] * p.W + j] >> (b & 31);
        out2[t] = (uint8_t)(v & 1u);
    } else if (out64 && t - t2 < (uint64_t)n_sel64 * p.B) {
        const uint64_t u = t - t2;
        const uint32_t b = (uint32_t)(u / n_sel64), i = (uint32_t)(u % n_sel64);
        out64[u] = p.v64[(size_t)ssa64[sel64 ? sel64[i] : i] * p.B + b];
    }
}

// rv_evaluate_batch_device, one thread per witness: the count of failing assertions and the first one's op-list index (the smaller
// of the two domains'; UINT64_MAX: none) as one 16-byte rv_eval_status.  f: the circuit's ordinal tables (its stream fields unread).
__global__ __launch_bounds__(256) void k_eval_status(EvalParams p, EvalFold f, rv_eval_status* __restrict__ out) {
    const uint32_t b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= p.B) return;
    rv_eval_status st;
    st.n_failed = p.n_failed[b];
    st.first_failed_op = min(ev_assert_op(f.rec2, f.op2, f.n2, p.first2[b]), ev_assert_op(f.rec64, f.op64, f.n64, p.first64[b]));
    out[b] = st;
}

// streaming evaluation, once per chunk, one thread per witness: the chunk's first failing assertion (the smaller op index of the two
// domains) becomes the stream's if it has none yet -- earlier chunks come first in program order -- and the chunk's count is added
__global__ __launch_bounds__(256) void k_eval_fold(EvalParams p, EvalFold f) {
    const uint32_t b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= p.B) return;
    const uint64_t x = min(ev_assert_op(f.rec2, f.op2, f.n2, p.first2[b]), ev_assert_op(f.rec64, f.op64, f.n64, p.first64[b]));
    if (x != UINT64_MAX && f.first_op[b] == UINT64_MAX) f.first_op[b] = f.op_base + x;
    f.total[b] += p.n_failed[b];
    p.n_failed[b] = 0;
    p.first2[b] = UINT32_MAX;
    p.first64[b] = UINT32_MAX;
}

// streaming evaluation: the carried wires' values of witnesses [b0, b0 + nb) -> [nb][n_gf2] bytes and [nb][n_z64] words
__global__ __launch_bounds__(256) void k_eval_stream_out(EvalParams p, uint32_t n_gf2, uint32_t n_z64, uint32_t b0, uint32_t nb,
                                                         uint8_t* __restrict__ out2, uint64_t* __restrict__ out64) {
    const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const uint64_t t2 = out2 ? (uint64_t)n_gf2 * nb : 0;
    if (t < t2) {
        const uint32_t b = b0 + (uint32_t)(t / n_gf2), w = (uint32_t)(t % n_gf2);
        out2[t] = (uint8_t)((p.val[(size_t)w * p.W + (b >> 5)] >> (b & 31)) & 1u);
    } else if (out64 && t - t2 < (uint64_t)n_z64 * nb) {
        const uint64_t u = t - t2;
        const uint32_t b = b0 + (uint32_t)(u / n_z64), w = (uint32_t)(u % n_z64);
        out64[u] = p.v64[(size_t)(1 + w) * p.B + b];
    }
}

inline unsigned blocks_for(uint64_t n, unsigned bs) { return (unsigned)((n + bs - 1) / bs); }

}  // namespace

void launch_eval_level(hipStream_t st, const EvalParams& p, const Gate* d_gates, uint32_t lo, uint32_t n2, const Gate64* d_gates64, uint32_t lo64,
                       uint32_t n64) {
    const uint64_t n = (uint64_t)n2 * p.W + (uint64_t)n64 * p.B;
    if (!n) return;
    hipLaunchKernelGGL(k_eval_level, dim3(blocks_for(n, 256)), dim3(256), 0, st, p, d_gates, lo, n2, d_gates64, lo64, n64);
}

void launch_eval_walk(hipStream_t st, const EvalParams& p, const Gate* d_gates, const LevelRange* d_lr, const Gate64* d_gates64, const uint32_t* d_ls64,
                      uint32_t n_levels, uint32_t S, uint32_t threads) {
    hipLaunchKernelGGL(k_eval_walk, dim3((p.W + S - 1) / S), dim3(threads), 0, st, p, d_gates, d_lr, d_gates64, d_ls64, n_levels, S);
}

void launch_eval_wit(hipStream_t st, const uint8_t* d_wit, size_t stride, uint32_t n, uint32_t B, uint32_t W, uint32_t* d_out) {
    const uint64_t t = (uint64_t)n * W;
    if (!t) return;
    hipLaunchKernelGGL(k_eval_wit, dim3(blocks_for(t, 256)), dim3(256), 0, st, d_wit, stride, n, B, W, d_out);
}

void launch_eval_out(hipStream_t st, const EvalParams& p, const WireForm* d_forms, uint32_t n_gf2, const uint32_t* d_ssa64, uint32_t n_z64,
                     uint8_t* d_out2, uint64_t* d_out64) {
    const uint64_t t = (d_out2 ? (uint64_t)n_gf2 * p.B : 0) + (d_out64 ? (uint64_t)n_z64 * p.B : 0);
    if (!t) return;
    hipLaunchKernelGGL(k_eval_out, dim3(blocks_for(t, 256)), dim3(256), 0, st, p, d_forms, n_gf2, d_ssa64, n_z64, d_out2, d_out64);
}

void launch_eval_out_sel(hipStream_t st, const EvalParams& p, const WireForm* d_forms, const uint32_t* d_sel2, uint32_t n_sel2, const uint32_t* d_ssa64,
                         const uint32_t* d_sel64, uint32_t n_sel64, uint8_t* d_out2, uint64_t* d_out64) {
    const uint64_t t = (d_out2 ? (uint64_t)n_sel2 * p.B : 0) + (d_out64 ? (uint64_t)n_sel64 * p.B : 0);
    if (!t) return;
    hipLaunchKernelGGL(k_eval_out_sel, dim3(blocks_for(t, 256)), dim3(256), 0, st, p, d_forms, d_sel2, n_sel2, d_ssa64, d_sel64, n_sel64, d_out2, d_out64);
}

void launch_eval_status(hipStream_t st, const EvalParams& p, const EvalFold& f, rv_eval_status* d_out) {
    hipLaunchKernelGGL(k_eval_status, dim3(blocks_for(p.B, 256)), dim3(256), 0, st, p, f, d_out);
}

void launch_eval_fold(hipStream_t st, const EvalParams& p, const EvalFold& f) {
    hipLaunchKernelGGL(k_eval_fold, dim3(blocks_for(p.B, 256)), dim3(256), 0, st, p, f);
}

void launch_eval_stream_out(hipStream_t st, const EvalParams& p, uint32_t n_gf2, uint32_t n_z64, uint32_t b0, uint32_t nb, uint8_t* d_out2,
                            uint64_t* d_out64) {
    const uint64_t t = (d_out2 ? (uint64_t)n_gf2 * nb : 0) + (d_out64 ? (uint64_t)n_z64 * nb : 0);
    if (!t) return;
    hipLaunchKernelGGL(k_eval_stream_out, dim3(blocks_for(t, 256)), dim3(256), 0, st, p, n_gf2, n_z64, b0, nb, d_out2, d_out64);
}

}  // namespace rv
