// see compile_dev.h
//
// (Z64 ops and mixed lists, RV_COMPILE_DEVICE_Z64, and B2A ops, RV_COMPILE_DEVICE_B2A: compile_mixed_device, at the end of this file.)
// The device compile of a whole GF(2) program at K = 1 (every XOR of two distinct rows materialised; the lazy-sum form's differences are
// with its kernels: value_lazy, and the LAZY instantiations of steps 3 and 5), in the steps of the host
// compiler (compile.cpp: run_pass, Builder, the (level, class) sort and the pipelining tables):
//   1. classify   one thread per op: validation (any error -> the flag word -> the host compiler), the counters Builder::g_* keep
//                 (masks, Mul, AssertZero, Input: one exclusive scan gives every gate's m / eo / ep / x), the ordinal tables
//   2. writers    the writes keyed by wire (stable LSD radix sort, op index as value); a read of wire w at op i resolves to the last
//                 write of w before i by binary search in w's segment -- none: the never-written wire, SSA 0 (single.rs:14-16);
//                 the same pass counts every value's reads (pass 1's `uses`) and each op's pending operands
//   3. levels     Kahn rounds over the op DAG (consumer CSR from the read counts): one bounded launch per round, the frontier of
//                 round r + 1 gathered per workgroup in LDS and appended while round r runs.  A value is (row = the op that wrote its row, or none;
//                 constant bit; the row's level), the rules of Builder::g_xor / g_xorc / g_andc / g_const / g_mul at lazy_k = 1
//   4. rows       computed rows numbered in program order after the zero row (a scan of the materialised XORs)
//   5. tables     (level, class) keys, a stable radix sort of the gates, the records written straight into the circuit's gate array,
//                 the LevelRange bounds, the per-level mask-block maxima and the online rows' levels (-> level_done_on)
// No kernel waits for another workgroup; every loop is bounded by the op count, the level count or a round cap.
//
// Chunk mode (a ChunkStart: one piece of a stream, compile_ops_seq's `chunk`): a read with no write before it in the piece resolves to
// the wire's carried row (producer -2 - wire instead of -1), the counters start at the ChunkStart's, nothing is dropped as unread, and
//   6. write-back  a flag scan over the wires (written; final form still reads a carried row) numbers the extra computed rows and the
//                  gates of the write-back level, which go straight to their places: the materialised carried forms are level 0's
//                  class 3, the write-backs the last level's, both in wire order -- no op gate has class 3 at K = 1
#include "compile_dev.h"

#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <functional>
#include <vector>

namespace rv {

namespace {

constexpr int TB = 256;           // threads per workgroup of every kernel here
constexpr int SI = 8;             // items per thread of the scans and the radix sort
constexpr int TILE = TB * SI;     // items per workgroup
constexpr uint32_t MAX_ROUNDS = 1u << 16;  // topological rounds before the host compiler takes over

// the counters of one op (compile.cpp Builder): ShareGen::next() calls, Mul gates, AssertZero gates, Input gates
struct C4 {
    uint32_t m, mul, as, in;
};
struct SumC4 {
    __device__ C4 operator()(const C4& a, const C4& b) const { return C4{a.m + b.m, a.mul + b.mul, a.as + b.as, a.in + b.in}; }
    static __device__ C4 id() { return C4{0, 0, 0, 0}; }
};
// what a streaming chunk adds to the kernels' numbering (all zero: a whole program)
struct Seeds {
    uint32_t chunk;    // 1: chunk mode
    uint32_t base;     // carried rows in front of the PRG rows (row_prg_base)
    uint32_t m0;       // ShareGen calls before the piece, modulo 128
    uint32_t on0, pre0;  // transcript rows in front of the piece's own
    uint32_t n_wbmat;  // carried forms materialised for the write-back level (level 0, class 3)
};
struct SumU32 {
    __device__ uint32_t operator()(uint32_t a, uint32_t b) const { return a + b; }
    static __device__ uint32_t id() { return 0; }
};
struct MaxU32 {
    __device__ uint32_t operator()(uint32_t a, uint32_t b) const { return a > b ? a : b; }
    static __device__ uint32_t id() { return 0; }
};

// ---- exclusive scan (reduce, scan of the workgroup sums, down-sweep) ----
template <class T, class Op>
__global__ __launch_bounds__(TB) void k_scan_up(const T* in, size_t n, T* sums) {
    Op op;
    __shared__ T sh[TB];
    const size_t base = (size_t)blockIdx.x * TILE + (size_t)threadIdx.x * SI;
    T acc = Op::id();
    for (int k = 0; k < SI; k++)
        if (base + k < n) acc = op(acc, in[base + k]);
    sh[threadIdx.x] = acc;
    __syncthreads();
    for (int s = TB / 2; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) sh[threadIdx.x] = op(sh[threadIdx.x], sh[threadIdx.x + s]);
        __syncthreads();
    }
    if (threadIdx.x == 0) sums[blockIdx.x] = sh[0];
}
template <class T, class Op>
__device__ T block_excl(T v, T* sh, T* total) {  // exclusive scan of one value per thread across the workgroup
    Op op;
    sh[threadIdx.x] = v;
    __syncthreads();
    for (int s = 1; s < TB; s <<= 1) {
        const T t = (int)threadIdx.x >= s ? sh[threadIdx.x - s] : Op::id();
        __syncthreads();
        sh[threadIdx.x] = op(sh[threadIdx.x], t);
        __syncthreads();
    }
    const T ex = threadIdx.x ? sh[threadIdx.x - 1] : Op::id();
    *total = sh[TB - 1];
    __syncthreads();
    return ex;
}
template <class T, class Op>
__global__ __launch_bounds__(TB) void k_scan_mid(T* sums, size_t nb, T* total) {
    Op op;
    __shared__ T sh[TB];
    T carry = Op::id();
    for (size_t c0 = 0; c0 < nb; c0 += TB) {
        const size_t i = c0 + threadIdx.x;
        T tot;
        const T ex = block_excl<T, Op>(i < nb ? sums[i] : Op::id(), sh, &tot);
        if (i < nb) sums[i] = op(carry, ex);
        carry = op(carry, tot);
    }
    if (threadIdx.x == 0 && total) *total = carry;
}
template <class T, class Op>
__global__ __launch_bounds__(TB) void k_scan_down(const T* in, T* out, size_t n, const T* sums) {
    Op op;
    __shared__ T sh[TB];
    const size_t base = (size_t)blockIdx.x * TILE + (size_t)threadIdx.x * SI;
    T v[SI];
    T acc = Op::id();
    for (int k = 0; k < SI; k++) {
        v[k] = base + k < n ? in[base + k] : Op::id();
        acc = op(acc, v[k]);
    }
    T tot;
    T run = op(sums[blockIdx.x], block_excl<T, Op>(acc, sh, &tot));
    for (int k = 0; k < SI; k++)
        if (base + k < n) {
            out[base + k] = run;
            run = op(run, v[k]);
        }
}

// ---- stable LSD radix sort of (key, value) pairs, 8 bits per pass ----
__global__ __launch_bounds__(TB) void k_rs_hist(const uint32_t* keys, size_t n, int shift, uint32_t* hist, uint32_t n_tiles) {
    __shared__ uint32_t h[256];
    h[threadIdx.x] = 0;
    __syncthreads();
    const size_t base = (size_t)blockIdx.x * TILE;
    for (int s = 0; s < SI; s++) {
        const size_t i = base + (size_t)s * TB + threadIdx.x;
        if (i < n) atomicAdd(&h[(keys[i] >> shift) & 255u], 1u);
    }
    __syncthreads();
    hist[(size_t)threadIdx.x * n_tiles + blockIdx.x] = h[threadIdx.x];
}
// items of a tile in order: sub-round s, then thread; the rank of an item among the equal digits before it comes from
// wavefront ballots (the lanes that share its digit) and the per-wavefront digit counts of the sub-round in LDS
__global__ __launch_bounds__(TB) void k_rs_scatter(const uint32_t* kin, const uint32_t* vin, uint32_t* kout, uint32_t* vout, size_t n, int shift,
                                                   const uint32_t* off, uint32_t n_tiles) {
    __shared__ uint32_t run[256];
    __shared__ uint32_t wc[TB / 64][256];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    run[threadIdx.x] = off[(size_t)threadIdx.x * n_tiles + blockIdx.x];
    const size_t base = (size_t)blockIdx.x * TILE;
    for (int s = 0; s < SI; s++) {
        for (int w = 0; w < TB / 64; w++) wc[w][threadIdx.x] = 0;
        __syncthreads();
        const size_t i = base + (size_t)s * TB + threadIdx.x;
        const bool valid = i < n;
        const uint32_t k = valid ? kin[i] : 0u;
        const uint32_t d = (k >> shift) & 255u;
        unsigned long long peers = __ballot(valid);
        for (int b = 0; b < 8; b++) {
            const unsigned long long bb = __ballot(valid && ((d >> b) & 1u));
            peers &= ((d >> b) & 1u) ? bb : ~bb;
        }
        const uint32_t rank = (uint32_t)__popcll(peers & ((1ull << lane) - 1ull));
        const uint32_t cnt = (uint32_t)__popcll(peers);
        if (valid && rank + 1 == cnt) wc[wave][d] = cnt;
        __syncthreads();
        if (valid) {
            uint32_t at = run[d] + rank;
            for (uint32_t w = 0; w < wave; w++) at += wc[w][d];
            kout[at] = k;
            vout[at] = vin[i];
        }
        __syncthreads();
        uint32_t add = 0;
        for (int w = 0; w < TB / 64; w++) add += wc[w][threadIdx.x];
        run[threadIdx.x] += add;
        __syncthreads();
    }
}

// ---- the op list ----
// The private ops of a B2A expansion (RV_COMPILE_DEVICE_B2A; k_z_expand writes them into the GF(2) list of a mixed compile, nobody
// else may): GF(2) records whose `reserved` word says PS_OP = writes no wire (sort key W), PS_A / PS_B = operand a / b names its
// producer by its place in the list instead of a wire.  A PS_OP AssertZero is Builder::g_reveal(recon = true): the gate is a G_RECON
// and has a value, a fresh computed row.
constexpr uint16_t PS_OP = 1, PS_A = 2, PS_B = 4;
constexpr uint32_t B2A_STEPS = 442, B2A_RECON0 = 378;  // SSA-producing steps of one B2A (run_pass); its first reconstruction
constexpr uint8_t ZOP_B2A = RV_OP_CONST + 1;           // the B2A's record in the Z64 list (a = its expansion's place in the GF(2) list)
__device__ inline bool is_recon(const rv_op& op) { return op.opcode == RV_OP_ASSERTZERO && (op.reserved & PS_OP); }
__device__ inline bool op_writes(uint32_t opc) { return opc != RV_OP_ASSERTZERO; }
__device__ inline int op_reads(uint32_t opc) {
    switch (opc) {
    case RV_OP_ADD: case RV_OP_SUB: case RV_OP_MUL: return 2;
    case RV_OP_ADDCONST: case RV_OP_SUBCONST: case RV_OP_MULCONST: case RV_OP_ASSERTZERO: return 1;
    default: return 0;
    }
}

// step 1: validation, counters, the wire sort's keys (a wire; W for ops that write none: they sort behind every wire)
// (pseudo: the list is a mixed compile's own and may hold the private ops of B2A expansions)
__global__ __launch_bounds__(TB) void k_cd_classify(const rv_op* ops, size_t n, uint32_t W, uint32_t pseudo, C4* cnt, uint32_t* keys, uint32_t* vals,
                                                    uint32_t* flag) {
    const size_t i = (size_t)blockIdx.x * TB + threadIdx.x;
    if (i >= n) return;
    const rv_op op = ops[i];
    bool bad = op.domain != RV_DOM_GF2 || (pseudo ? (op.reserved & ~(PS_OP | PS_A | PS_B)) != 0 : op.reserved != 0) || op.opcode > RV_OP_CONST;
    const int nr = bad ? 0 : op_reads(op.opcode);
    const bool wr = !bad && op_writes(op.opcode) && !(op.reserved & PS_OP);
    if (wr && op.dst >= W) bad = true;
    if (nr >= 1 && !(op.reserved & PS_A) && op.a >= W) bad = true;
    if (nr >= 2 && !(op.reserved & PS_B) && op.b >= W) bad = true;
    if (bad) atomicOr(flag, 1u);
    C4 c{0, 0, 0, 0};
    if (!bad) {
        if (op.opcode == RV_OP_INPUT) c.m = 1, c.in = 1;
        else if (op.opcode == RV_OP_RANDOM) c.m = 1;
        else if (op.opcode == RV_OP_MUL) c.m = 2, c.mul = 1;
        else if (op.opcode == RV_OP_ASSERTZERO) c.as = 1;
    }
    cnt[i] = c;
    keys[i] = wr ? op.dst : W;
    vals[i] = (uint32_t)i;
}

// the ordinal tables: reconstruction ordinal -> online row, input ordinal -> online row, the AssertZero ops
// (b2a_base: where the n_b2a expansions start in the list, ascending.  Their reconstructions count in c.as like AssertZero ops but are
// not in the AssertZero tables: 64 per expansion in front of op i come off its ordinal there)
__global__ __launch_bounds__(TB) void k_cd_ordinals(const rv_op* ops, size_t n, const C4* cx, uint32_t on0, uint32_t* rec_rows, uint32_t* in_rows,
                                                    uint32_t* as_rec, uint64_t* as_op, const uint32_t* orig, const uint32_t* b2a_base, uint32_t n_b2a) {
    const size_t i = (size_t)blockIdx.x * TB + threadIdx.x;
    if (i >= n) return;
    const rv_op op = ops[i];
    const uint32_t opc = op.opcode;
    const C4 c = cx[i];
    const uint32_t eo = on0 + c.in + c.mul + c.as, x = c.mul + c.as;
    if (opc == RV_OP_INPUT) in_rows[c.in] = eo;
    if (opc == RV_OP_MUL || opc == RV_OP_ASSERTZERO) rec_rows[x] = eo;
    if (opc == RV_OP_ASSERTZERO && !is_recon(op)) {
        uint32_t a = 0, b = n_b2a;
        while (a < b) {  // (expansions that start before op i; at most 32 steps)
            const uint32_t mid = a + (b - a) / 2;
            if (b2a_base[mid] < i) a = mid + 1;
            else b = mid;
        }
        const uint32_t k = c.as - 64u * a;
        as_rec[k] = x;
        as_op[k] = orig ? orig[i] : i;  // (orig: the ops are the GF(2) ops of a mixed list, orig[i] = op i's place in it)
    }
}

// step 2: each wire's segment of the sorted writes
__global__ __launch_bounds__(TB) void k_cd_segs(const uint32_t* sk, size_t n, uint32_t W, uint32_t* seg_lo, uint32_t* seg_hi) {
    const size_t p = (size_t)blockIdx.x * TB + threadIdx.x;
    if (p >= n) return;
    const uint32_t k = sk[p];
    if (k >= W) return;
    if (p == 0 || sk[p - 1] != k) seg_lo[k] = (uint32_t)p;
    if (p + 1 == n || sk[p + 1] != k) seg_hi[k] = (uint32_t)p + 1;
}
__device__ inline int last_writer(const uint32_t* sv, const uint32_t* seg_lo, const uint32_t* seg_hi, uint32_t w, uint32_t i) {
    uint32_t lo = seg_lo[w], a = lo, b = seg_hi[w];
    while (a < b) {  // (at most 32 steps)
        const uint32_t mid = a + (b - a) / 2;
        if (sv[mid] < i) a = mid + 1;
        else b = mid;
    }
    return a > lo ? (int)sv[a - 1] : -1;
}
// the producer of every operand (-1: the never-written wire; chunk mode: -2 - w, wire w's carried row), read counts, pending operands
__global__ __launch_bounds__(TB) void k_cd_resolve(const rv_op* ops, size_t n, const uint32_t* sv, const uint32_t* seg_lo, const uint32_t* seg_hi,
                                                   uint32_t chunk, int2* prod, uint32_t* uses, uint32_t* rem) {
    const size_t i = (size_t)blockIdx.x * TB + threadIdx.x;
    if (i >= n) return;
    const rv_op op = ops[i];
    const int nr = op_reads(op.opcode);
    int2 p = make_int2(-1, -1);
    // (a private op of a B2A expansion names the steps of its own expansion by their places; its reads of the source wires are
    // searched like any other: no step of an expansion writes a wire, so every place in it sees the B2A's own last writers)
    if (nr >= 1) p.x = (op.reserved & PS_A) ? (int)op.a : last_writer(sv, seg_lo, seg_hi, op.a, (uint32_t)i);
    if (nr >= 2) p.y = (op.reserved & PS_B) ? (int)op.b : last_writer(sv, seg_lo, seg_hi, op.b, (uint32_t)i);
    if (chunk) {
        if (nr >= 1 && p.x < 0) p.x = -2 - (int)op.a;
        if (nr >= 2 && p.y < 0) p.y = -2 - (int)op.b;
    }
    uint32_t r = 0;
    if (p.x >= 0) atomicAdd(&uses[p.x], 1u), r++;
    if (p.y >= 0) atomicAdd(&uses[p.y], 1u), r++;
    prod[i] = p;
    rem[i] = r;
}
__global__ __launch_bounds__(TB) void k_cd_consumers(const int2* prod, size_t n, const uint32_t* cons_off, uint32_t* cursor, uint32_t* cons) {
    const size_t i = (size_t)blockIdx.x * TB + threadIdx.x;
    if (i >= n) return;
    const int2 p = prod[i];
    if (p.x >= 0) cons[cons_off[p.x] + atomicAdd(&cursor[p.x], 1u)] = (uint32_t)i;
    if (p.y >= 0) cons[cons_off[p.y] + atomicAdd(&cursor[p.y], 1u)] = (uint32_t)i;
}
// round 0's frontier: the ops with no pending operand
__global__ __launch_bounds__(TB) void k_cd_front0(const uint32_t* rem, size_t n, uint32_t* frontier, uint2* rounds) {
    const size_t i = (size_t)blockIdx.x * TB + threadIdx.x;
    if (i >= n) return;
    if (rem[i] == 0) frontier[atomicAdd(&rounds[0].y, 1u)] = (uint32_t)i;
}

// a value: x = the op that wrote its row (-1: a constant; -2 - w: wire w's carried row, there before level 0),
// y = (level of that row + 1) << 1 | constant bit
__device__ inline int2 val_of(const int2* V, int p) { return p < 0 ? make_int2(p, 0) : V[p]; }
__device__ inline int lvl_of(int2 v) { return (v.y >> 1) - 1; }
__device__ inline bool is_row(int2 v) { return v.x != -1; }

// ---- the lazy-sum form (force_lazy_k = RV_LIN_K; whole programs only) ----
// A value is a Lin of compile.cpp: x, y, z = up to RV_LIN_K rows in the host compiler's order, w = count | constant bit << 2 (the
// value of a materialised sum also keeps that gate's row count, << 8, for the statistics and the class keys).  A row is named by the
// op that wrote it, with ROW_COMP set when that op is a materialised sum: the host compiler sorts PRG rows (mask index) before
// computed rows (COMP | index), and both indices grow in op order, so comparing these names compares its row numbers.
// A row's level is glvl of its op; a never-written wire is the empty form.
static_assert(RV_LIN_K == 3, "a lazy value holds three rows");
constexpr uint32_t ROW_COMP = 1u << 30;  // (n_ops < 2^28)
__device__ inline uint4 form_of(const uint4* V3, int p) { return p < 0 ? make_uint4(0, 0, 0, 0) : V3[p]; }
__device__ inline uint32_t form_n(const uint4& F) { return F.w & 3u; }
__device__ inline uint32_t form_c(const uint4& F) { return (F.w >> 2) & 1u; }
__device__ inline uint32_t form_row(const uint4& F, int k) { return k == 0 ? F.x : k == 1 ? F.y : F.z; }
__device__ inline int form_lvl(const uint4& F, const int* glvl) {
    const uint32_t n = form_n(F);
    int l = -1;
    if (n > 0) l = max(l, glvl[F.x & ~ROW_COMP]);
    if (n > 1) l = max(l, glvl[F.y & ~ROW_COMP]);
    if (n > 2) l = max(l, glvl[F.z & ~ROW_COMP]);
    return l;
}
// Builder::g_xor's symmetric difference of two sorted row lists (x ^ x = 0): at most 6 rows, one or two consumed per step
__device__ inline int form_xor(const uint4& A, const uint4& B, uint32_t (&rows)[2 * RV_LIN_K]) {
    const int na = (int)form_n(A), nb = (int)form_n(B);
    int i = 0, j = 0, n = 0;
#pragma unroll
    for (int k = 0; k < 2 * RV_LIN_K; k++) rows[k] = 0;
#pragma unroll
    for (int t = 0; t < 2 * RV_LIN_K; t++) {
        if (i < na || j < nb) {
            const uint32_t x = i < na ? form_row(A, i) : 0xFFFFFFFFu, y = j < nb ? form_row(B, j) : 0xFFFFFFFFu;
            if (x == y) {
                i++, j++;
            } else {
                const uint32_t v = min(x, y);
                i += x < y, j += y < x;
#pragma unroll
                for (int k = 0; k < 2 * RV_LIN_K; k++)
                    if (n == k) rows[k] = v;
                n++;
            }
        }
    }
    return n;
}

// the value of op i, the level of its gate (-1: none) and whether it is a materialised sum: the rules of Builder::g_xor / g_xorc /
// g_andc / g_const / g_mul at lazy_k = 1 ...
__device__ inline int2 value_k1(const rv_op& op, uint32_t i, int2 p, uint32_t chunk, const uint32_t* uses, const int2* V, int* gl, uint32_t* mt) {
    const int2 A = val_of(V, p.x), B = val_of(V, p.y);
    const int cb = (int)(op.imm & 1);
    int2 out = make_int2(-1, 0);
    switch (op.opcode) {
    case RV_OP_INPUT:
    case RV_OP_RANDOM:
        *gl = 0;
        out = make_int2((int)i, 1 << 1);
        break;
    case RV_OP_CONST:
        out = make_int2(-1, cb);
        break;
    case RV_OP_ADD:
    case RV_OP_SUB:
        if (A.x == B.x) out = make_int2(-1, (A.y ^ B.y) & 1);       // x ^ x = 0 (or two constants)
        else if (!is_row(A)) out = make_int2(B.x, B.y ^ (A.y & 1));  // a constant plus a row: the row
        else if (!is_row(B)) out = make_int2(A.x, A.y ^ (B.y & 1));
        else if (!chunk && uses[i] == 0) out = make_int2(-1, 0);    // an unread sum is dropped (a chunk counts no reads)
        else {                                                      // two rows: a G_XORK
            *gl = max(lvl_of(A), lvl_of(B)) + 1;
            out = make_int2((int)i, (*gl + 1) << 1);
            *mt = 1;
        }
        break;
    case RV_OP_ADDCONST:
    case RV_OP_SUBCONST:
        out = make_int2(A.x, A.y ^ cb);
        break;
    case RV_OP_MULCONST:
        out = cb ? A : make_int2(-1, 0);
        break;
    case RV_OP_MUL:
        *gl = max(lvl_of(A), lvl_of(B)) + 1;
        out = make_int2((int)i, (*gl + 1) << 1);
        break;
    default:  // AssertZero; a B2A's reconstruction also has a value, its own computed row
        *gl = lvl_of(A) + 1;
        if (op.reserved & PS_OP) {
            out = make_int2((int)i, (*gl + 1) << 1);
            *mt = 1;
        }
        break;
    }
    return out;
}
// ... and at lazy_k = RV_LIN_K, lazy_slack = 1, balance = 0 (a forced compile): a sum of n rows read f times stays symbolic while
// f x (n - 1) extra operand rows cost no more than the n reads and one write of materialising it
__device__ inline uint4 value_lazy(const rv_op& op, uint32_t i, int2 p, const uint32_t* uses, const uint4* V3, const int* glvl, int* gl, uint32_t* mt) {
    const uint4 A = form_of(V3, p.x), B = form_of(V3, p.y);
    const uint32_t cb = (uint32_t)(op.imm & 1);
    const uint4 none = make_uint4(0, 0, 0, 0);
    uint4 out = none;
    switch (op.opcode) {
    case RV_OP_INPUT:
    case RV_OP_RANDOM:
        *gl = 0;
        out = make_uint4(i, 0, 0, 1);
        break;
    case RV_OP_CONST:
        out = make_uint4(0, 0, 0, cb << 2);
        break;
    case RV_OP_ADD:
    case RV_OP_SUB: {
        uint32_t rows[2 * RV_LIN_K];
        const uint32_t n = (uint32_t)form_xor(A, B, rows), c = form_c(A) ^ form_c(B);
        const uint32_t f = uses[i];
        if (f == 0) break;  // an unread sum is dropped
        if (n <= 1 || (n <= (uint32_t)RV_LIN_K && (uint64_t)f * (n - 1) <= (uint64_t)n + 1)) {
            out = make_uint4(rows[0], rows[1], rows[2], n | c << 2);
        } else {  // one G_XORK of n rows; the constant goes into the gate
            int l = -1;
#pragma unroll
            for (int k = 0; k < 2 * RV_LIN_K; k++)
                if ((uint32_t)k < n) l = max(l, glvl[rows[k] & ~ROW_COMP]);
            *gl = l + 1;
            *mt = 1;
            out = make_uint4(i | ROW_COMP, 0, 0, 1u | n << 8);
        }
        break;
    }
    case RV_OP_ADDCONST:
    case RV_OP_SUBCONST:
        out = make_uint4(A.x, A.y, A.z, (A.w & 7u) ^ cb << 2);
        break;
    case RV_OP_MULCONST:
        out = cb ? make_uint4(A.x, A.y, A.z, A.w & 7u) : none;
        break;
    case RV_OP_MUL:
        *gl = max(form_lvl(A, glvl), form_lvl(B, glvl)) + 1;
        out = make_uint4(i, 0, 0, 1);
        break;
    default:  // AssertZero; a B2A's reconstruction also has a value, its own computed row
        *gl = form_lvl(A, glvl) + 1;
        if (op.reserved & PS_OP) {
            out = make_uint4(i | ROW_COMP, 0, 0, 1);
            *mt = 1;
        }
        break;
    }
    return out;
}

// a Z64 op's level (run_pass, case RV_DOM_Z64): Input, Random and Const 0, every other gate one above its deepest operand; SSA 0 and
// a chunk's carried slots (p < 0) count as -1
// (a B2A: one above its deepest reconstruction, which k_z_b2a_levels wrote before the rounds)
__device__ inline int level_z64(const rv_op& op, uint32_t i, int2 p, const int* glvl) {
    if (op.opcode == ZOP_B2A) return glvl[i];
    if (op_reads(op.opcode) == 0) return 0;
    return max(p.x >= 0 ? glvl[p.x] : -1, p.y >= 0 ? glvl[p.y] : -1) + 1;
}

// step 3: one round.  rounds[r] = {first frontier slot, count}; the ops whose last pending operand this round resolves form
// round r + 1's frontier.  FORM_LAZY: the values are lazy sums in V3 (V unused); FORM_K1: one row or a constant in V (V3 unused);
// FORM_Z64: Z64 ops, which have a level and no value (V, V3, mat unused).
enum { FORM_K1 = 0, FORM_LAZY = 1, FORM_Z64 = 2 };
template <int FORM>
__global__ __launch_bounds__(TB) void k_cd_round(uint32_t r, uint32_t chunk, const rv_op* ops, const int2* prod, const uint32_t* uses, const uint32_t* cons_off,
                                                 const uint32_t* cons, uint32_t* rem, int2* V, uint4* V3, int* glvl, uint32_t* mat, uint32_t* frontier,
                                                 uint2* rounds) {
    // the next frontier is gathered in LDS and appended with one global atomic per workgroup (65 536 appends to one counter per
    // round of the benchmark circuit otherwise); what does not fit the LDS queue is appended one by one
    constexpr uint32_t FQ = 2048;
    __shared__ uint32_t q[FQ];
    __shared__ uint32_t qn, qbase;
    if (threadIdx.x == 0) qn = 0;
    __syncthreads();
    const uint2 R = rounds[r];
    const uint32_t nb = R.x + R.y;
    if (blockIdx.x == 0 && threadIdx.x == 0) rounds[r + 1].x = nb;
    for (uint32_t t = blockIdx.x * TB + threadIdx.x; t < R.y; t += gridDim.x * TB) {
        const uint32_t i = frontier[R.x + t];
        const rv_op op = ops[i];
        const int2 p = prod[i];
        int gl = -1;
        uint32_t mt = 0;
        if constexpr (FORM == FORM_Z64) gl = level_z64(op, i, p, glvl);
        else if constexpr (FORM == FORM_LAZY) V3[i] = value_lazy(op, i, p, uses, V3, glvl, &gl, &mt);
        else V[i] = value_k1(op, i, p, chunk, uses, V, &gl, &mt);
        glvl[i] = gl;
        if constexpr (FORM != FORM_Z64) mat[i] = mt;
        const uint32_t c0 = cons_off[i], c1 = c0 + uses[i];
        for (uint32_t k = c0; k < c1; k++) {
            const uint32_t c = cons[k];
            if (atomicSub(&rem[c], 1u) == 1u) {
                const uint32_t s = atomicAdd(&qn, 1u);
                if (s < FQ) q[s] = c;
                else frontier[nb + atomicAdd(&rounds[r + 1].y, 1u)] = c;
            }
        }
    }
    __syncthreads();
    const uint32_t m = min(qn, FQ);
    if (threadIdx.x == 0 && m) qbase = atomicAdd(&rounds[r + 1].y, m);
    __syncthreads();
    for (uint32_t j = threadIdx.x; j < m; j += TB) frontier[nb + qbase + j] = q[j];
}

struct DevStats {
    int max_level;
    uint32_t n_gates, n_mat, pad;
    unsigned long long operand_rows;
};
// the gate count, materialised XORs, levels and operand rows (one atomic per workgroup and counter)
template <bool LAZY>
__global__ __launch_bounds__(TB) void k_cd_stats(const rv_op* ops, size_t n, const int2* prod, const int2* V, const uint4* V3, const int* glvl,
                                                 const uint32_t* mat, DevStats* st) {
    __shared__ int sl[TB];
    __shared__ uint32_t sg[TB], sm[TB], so[TB];
    const size_t i = (size_t)blockIdx.x * TB + threadIdx.x;
    int l = -1;
    uint32_t g = 0, m = 0, o = 0;
    if (i < n) {
        l = glvl[i];
        g = l >= 0;
        m = mat[i];
        const uint32_t opc = ops[i].opcode;
        const int2 p = prod[i];
        if constexpr (LAZY) {  // the rows of the operand forms; a materialised sum's own
            if (opc == RV_OP_MUL) o = form_n(form_of(V3, p.x)) + form_n(form_of(V3, p.y));
            else if (opc == RV_OP_ASSERTZERO) o = form_n(form_of(V3, p.x));
            else if (m) o = V3[i].w >> 8;
        } else {
            if (opc == RV_OP_MUL) o = is_row(val_of(V, p.x)) + is_row(val_of(V, p.y));
            else if (opc == RV_OP_ASSERTZERO) o = is_row(val_of(V, p.x));
            else if (m) o = 2;
        }
    }
    sl[threadIdx.x] = l, sg[threadIdx.x] = g, sm[threadIdx.x] = m, so[threadIdx.x] = o;
    __syncthreads();
    for (int s = TB / 2; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) {
            sl[threadIdx.x] = max(sl[threadIdx.x], sl[threadIdx.x + s]);
            sg[threadIdx.x] += sg[threadIdx.x + s];
            sm[threadIdx.x] += sm[threadIdx.x + s];
            so[threadIdx.x] += so[threadIdx.x + s];
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        atomicMax(&st->max_level, sl[0]);
        atomicAdd(&st->n_gates, sg[0]);
        atomicAdd(&st->n_mat, sm[0]);
        atomicAdd(&st->operand_rows, (unsigned long long)so[0]);
    }
}

// step 5: the (level, class) key of every gate (LevelRange classes: Mul of one-base operands 0, other Mul 1, two-row Xor 2,
// any other Xor 3 -- lazy sums only --, the rest 4; ops without a gate get `sentinel`, behind every gate)
template <bool LAZY>
__global__ __launch_bounds__(TB) void k_cd_keys(const rv_op* ops, size_t n, const int2* prod, const int2* V, const uint4* V3, const int* glvl,
                                                const uint32_t* mat, uint32_t sentinel, uint32_t* keys, uint32_t* vals) {
    const size_t i = (size_t)blockIdx.x * TB + threadIdx.x;
    if (i >= n) return;
    const int l = glvl[i];
    uint32_t key = sentinel;
    if (l >= 0) {
        const uint32_t opc = ops[i].opcode;
        uint32_t cls = 4;
        if (opc == RV_OP_MUL) {
            const int2 p = prod[i];
            if constexpr (LAZY) cls = (form_n(form_of(V3, p.x)) == 1 && form_n(form_of(V3, p.y)) == 1) ? 0u : 1u;
            else cls = (is_row(val_of(V, p.x)) && is_row(val_of(V, p.y))) ? 0u : 1u;
        } else if (opc != RV_OP_ASSERTZERO && mat[i]) {  // (a reconstruction has a computed row too: class 4)
            cls = 2;
            if constexpr (LAZY) cls = (V3[i].w >> 8) == 2 ? 2u : 3u;
        }
        key = (uint32_t)l * 5u + cls;
    }
    keys[i] = key;
    vals[i] = (uint32_t)i;
}
// pos[k] = first sorted gate with key >= k, k in [0, n_buckets]
__global__ __launch_bounds__(TB) void k_cd_bounds(const uint32_t* sk, size_t n_gates, uint32_t n_buckets, uint32_t* pos) {
    const size_t p = (size_t)blockIdx.x * TB + threadIdx.x;
    if (p > n_gates) return;
    const uint32_t lo = p == 0 ? 0u : sk[p - 1] + 1u;
    const uint32_t hi = p == n_gates ? n_buckets : sk[p];
    for (uint32_t k = lo; k <= hi; k++) pos[k] = (uint32_t)p;
}

// a value's row as a share row index: a chunk's carried rows, the PRG rows (Input / Random: m, Mul: m + 1), then the computed rows
// (zero row first)
__device__ inline uint32_t row_index(const rv_op* ops, const C4* cx, const uint32_t* comp, const Seeds& s, uint32_t pad, int q) {
    if (q == -1) return s.base + pad;
    if (q < -1) return (uint32_t)(-2 - q);
    const uint32_t opc = ops[q].opcode;
    if (opc == RV_OP_MUL) return s.base + s.m0 + cx[q].m + 1;
    if (opc == RV_OP_INPUT || opc == RV_OP_RANDOM) return s.base + s.m0 + cx[q].m;
    return s.base + pad + 1 + comp[q];
}
// the host compiler sorts a sum's rows as it names them before the final numbering: PRG rows, carried rows, computed rows
__device__ inline uint32_t row_rank(const Seeds& s, uint32_t pad, uint32_t row) { return row < s.base ? 1u : row >= s.base + pad ? 2u : 0u; }
__device__ inline uint32_t wave_max_u32(uint32_t v) {
    for (int s = 32; s > 0; s >>= 1) v = max(v, (uint32_t)__shfl_xor((int)v, s));
    return v;
}
// the gate records in (level, class, program) order, the per-level mask blocks and the online rows' levels
// (pad: the PRG rows, whole cipher blocks; a gate with key >= 4 sits behind the chunk's materialised carried forms)
// LAZY: Builder::fill of whole forms (up to RV_LIN_K rows per operand), a materialised sum of up to 2 RV_LIN_K rows
template <bool LAZY>
__global__ __launch_bounds__(TB) void k_cd_gates(const uint32_t* sk, const uint32_t* sv, size_t n_gates, const rv_op* ops, const int2* prod, const int2* V,
                                                 const uint4* V3, const C4* cx, const uint32_t* comp, Seeds s, uint32_t pad, Gate* gates,
                                                 uint32_t* need_raw, uint32_t* on_lvl) {
    const size_t p = (size_t)blockIdx.x * TB + threadIdx.x;
    const bool valid = p < n_gates;
    uint32_t l = 0, need = 0;
    if (valid) {
        l = sk[p] / 5u;
        const uint32_t i = sv[p];
        const rv_op op = ops[i];
        const C4 c = cx[i];
        const int2 pr = prod[i];
        int2 A = make_int2(-1, 0), B = A;
        uint4 FA = make_uint4(0, 0, 0, 0), FB = FA;
        if constexpr (LAZY) FA = form_of(V3, pr.x), FB = form_of(V3, pr.y);
        else A = val_of(V, pr.x), B = val_of(V, pr.y);
        const uint32_t e = c.in + c.mul + c.as, x = c.mul + c.as;  // e: the online row among the piece's own
        const uint32_t eo = s.on0 + e, m = s.m0 + c.m, zero = s.base + pad;
        Gate g;
        g.dst = s.base, g.m = s.base, g.eo = 0, g.ep = 0, g.x = 0;  // (the host compiler's unused fields: PRG row 0 after the carried rows)
        for (int k = 0; k < RV_LIN_K; k++) g.a[k] = zero, g.b[k] = zero;
        switch (op.opcode) {
        case RV_OP_INPUT:
            g.op = G_INPUT;
            g.m = g.dst = s.base + m;
            g.eo = eo;
            g.x = c.in;
            need = m / 128 + 1;
            on_lvl[e] = l;
            break;
        case RV_OP_RANDOM:
            g.op = G_RANDOM;
            g.m = g.dst = s.base + m;
            need = m / 128 + 1;
            break;
        case RV_OP_MUL: {
            if constexpr (LAZY) {
                const uint32_t na = form_n(FA), nb = form_n(FB);
                g.op = G_MUL | na << 8 | nb << 12 | form_c(FA) << 16 | form_c(FB) << 17;
                for (int k = 0; k < RV_LIN_K; k++) {
                    if ((uint32_t)k < na) g.a[k] = row_index(ops, cx, comp, s, pad, (int)(form_row(FA, k) & ~ROW_COMP));
                    if ((uint32_t)k < nb) g.b[k] = row_index(ops, cx, comp, s, pad, (int)(form_row(FB, k) & ~ROW_COMP));
                }
            } else {
                const uint32_t na = is_row(A), nb = is_row(B);
                g.op = G_MUL | na << 8 | nb << 12 | (uint32_t)(A.y & 1) << 16 | (uint32_t)(B.y & 1) << 17;
                if (na) g.a[0] = row_index(ops, cx, comp, s, pad, A.x);
                if (nb) g.b[0] = row_index(ops, cx, comp, s, pad, B.x);
            }
            g.m = s.base + m;
            g.dst = s.base + m + 1;
            g.eo = eo;
            g.ep = s.pre0 + c.mul;
            g.x = x;
            need = (m + 1) / 128 + 1;
            on_lvl[e] = l;
            break;
        }
        case RV_OP_ASSERTZERO: {
            const uint32_t gop = is_recon(op) ? G_RECON : G_ASSERT;
            if (gop == G_RECON) g.dst = zero + 1 + comp[i];
            if constexpr (LAZY) {
                const uint32_t na = form_n(FA);
                g.op = gop | na << 8 | form_c(FA) << 16;
                for (int k = 0; k < RV_LIN_K; k++)
                    if ((uint32_t)k < na) g.a[k] = row_index(ops, cx, comp, s, pad, (int)(form_row(FA, k) & ~ROW_COMP));
            } else {
                const uint32_t na = is_row(A);
                g.op = gop | na << 8 | (uint32_t)(A.y & 1) << 16;
                if (na) g.a[0] = row_index(ops, cx, comp, s, pad, A.x);
            }
            g.eo = eo;
            g.x = x;
            on_lvl[e] = l;
            break;
        }
        default: {  // a materialised Add / Sub: its two rows in the host compiler's order
            if constexpr (LAZY) {  // (Builder::materialise: the first RV_LIN_K rows in a[], the rest in b[], the constant in the gate)
                uint32_t rows[2 * RV_LIN_K];
                const uint32_t nr = (uint32_t)form_xor(FA, FB, rows), na = min(nr, (uint32_t)RV_LIN_K);
                g.op = G_XORK | na << 8 | (nr - na) << 12 | (form_c(FA) ^ form_c(FB)) << 16;
#pragma unroll
                for (int k = 0; k < RV_LIN_K; k++) {
                    if ((uint32_t)k < nr) g.a[k] = row_index(ops, cx, comp, s, pad, (int)(rows[k] & ~ROW_COMP));
                    if ((uint32_t)(RV_LIN_K + k) < nr) g.b[k] = row_index(ops, cx, comp, s, pad, (int)(rows[RV_LIN_K + k] & ~ROW_COMP));
                }
                g.dst = zero + 1 + comp[i];
                break;
            }
            const uint32_t ra = row_index(ops, cx, comp, s, pad, A.x), rb = row_index(ops, cx, comp, s, pad, B.x);
            const uint32_t ka = row_rank(s, pad, ra), kb = row_rank(s, pad, rb);
            const bool a_first = ka < kb || (ka == kb && ra < rb);
            g.op = G_XORK | 2u << 8 | (uint32_t)((A.y ^ B.y) & 1) << 16;
            g.a[0] = a_first ? ra : rb;
            g.a[1] = a_first ? rb : ra;
            g.dst = zero + 1 + comp[i];
            break;
        }
        }
        gates[p + (sk[p] >= 4u ? s.n_wbmat : 0u)] = g;
    }
    // a wavefront's gates mostly share a level: one atomic for them
    const uint32_t l0 = (uint32_t)__shfl((int)l, 0);
    if (__all(!valid || l == l0)) {
        const uint32_t m = wave_max_u32(need);
        if ((threadIdx.x & 63u) == 0 && m) atomicMax(&need_raw[l0], m);
    } else if (valid && need) {
        atomicMax(&need_raw[l], need);
    }
}
// step 6 (chunk mode).  Per wire: m = the piece wrote it, mul = its final form still reads a carried row (materialised first: two wires
// swapped by a piece must not race), as = the final form has a row (else it is a constant); lastw = the op that wrote it last.
constexpr uint32_t NO_WRITER = 0xFFFFFFFFu;
__global__ __launch_bounds__(TB) void k_cd_wb_flags(const uint32_t* sv, const uint32_t* seg_lo, const uint32_t* seg_hi, uint32_t W, const int2* V, C4* fl,
                                                    uint32_t* lastw) {
    const size_t w = (size_t)blockIdx.x * TB + threadIdx.x;
    if (w >= W) return;
    C4 f{0, 0, 0, 0};
    uint32_t q = NO_WRITER;
    if (seg_hi[w] > seg_lo[w]) {
        q = sv[seg_hi[w] - 1];
        const int2 v = V[q];
        f.m = 1;
        f.mul = v.x < -1;
        f.as = is_row(v);
    }
    fl[w] = f;
    lastw[w] = q;
}
// fx: the exclusive scan of the flags.  The materialised carried forms take the computed rows after the ops' own (n_mat of them) and
// level 0's class 3 (from *pos3; null: the piece has no op gate); the write-backs follow every other gate (from wb_at).
__global__ __launch_bounds__(TB) void k_cd_wb_gates(const uint32_t* lastw, const C4* fx, uint32_t W, const rv_op* ops, const int2* V, const C4* cx,
                                                    const uint32_t* comp, Seeds s, uint32_t pad, uint32_t n_mat, const uint32_t* pos3, uint32_t wb_at,
                                                    Gate* gates) {
    const size_t w = (size_t)blockIdx.x * TB + threadIdx.x;
    if (w >= W) return;
    const uint32_t q = lastw[w];
    if (q == NO_WRITER) return;
    const C4 r = fx[w];
    const int2 v = V[q];
    const uint32_t zero = s.base + pad;
    Gate g;
    g.op = G_XORK, g.dst = 0, g.m = s.base, g.eo = 0, g.ep = 0, g.x = 0;
    for (int k = 0; k < RV_LIN_K; k++) g.a[k] = zero, g.b[k] = zero;
    uint32_t row = zero, n = 0, c = (uint32_t)(v.y & 1);
    if (v.x < -1) {
        g.op = G_XORK | 1u << 8 | c << 16;
        g.a[0] = (uint32_t)(-2 - v.x);
        g.dst = zero + 1 + n_mat + r.mul;
        gates[(pos3 ? *pos3 : 0u) + r.mul] = g;
        row = g.dst, n = 1, c = 0;
    } else if (v.x >= 0) {
        row = row_index(ops, cx, comp, s, pad, v.x), n = 1;
    }
    g.op = G_XORK | n << 8 | c << 16;
    g.a[0] = row;
    g.dst = (uint32_t)w;
    gates[wb_at + r.m] = g;
}
// level_done_on[l] = online rows e whose prefix maximum of levels is <= l; pm = exclusive prefix maximum of on_lvl (n_on + 1 entries)
__global__ __launch_bounds__(TB) void k_cd_done_on(const uint32_t* pm, const uint32_t* on_lvl, size_t n_on, uint32_t n_levels, uint32_t* done_on) {
    const size_t e = (size_t)blockIdx.x * TB + threadIdx.x;
    if (e > n_on) return;
    const uint32_t lo = pm[e];
    const uint32_t hi = e == n_on ? n_levels : max(pm[e], on_lvl[e]);
    for (uint32_t l = lo; l < hi && l < n_levels; l++) done_on[l] = (uint32_t)e;
}

inline uint32_t blocks(size_t n, size_t per) { return (uint32_t)std::max<size_t>(1, (n + per - 1) / per); }
inline int bit_len(uint64_t v) {
    int b = 0;
    while (v) b++, v >>= 1;
    return b;
}

// device allocations of one compile, given back (after a stream sync) when it ends.  Per op, beside the caller's 24-byte op and the
// 48-byte gate records that stay with the circuit: counters 16, two key / value pairs of the sorts 16, producers 8, read counts,
// pending operands, consumer offsets and cursors 16, consumers 8, value 8 (the lazy-sum form: 16), level, materialised flag, frontier
// and computed-row index 16, the sorts' histograms 0.5: 89 bytes (lazy sums: 97); 8 bytes per wire for the writer segments, and a chunk
// 20 more for its write-back flags and last writers
struct Scratch {
    const DevAlloc& A;
    hipStream_t st;
    std::vector<void*> ps;
    bool failed = false;
    Scratch(const DevAlloc& a, hipStream_t s) : A(a), st(s) {}
    template <class T>
    T* get(size_t count) {
        void* p = nullptr;
        if (failed || A.alloc(A.self, std::max<size_t>(count, 1) * sizeof(T), &p) != RV_OK) {
            failed = true;
            return nullptr;
        }
        ps.push_back(p);
        return (T*)p;
    }
    void keep(void* p) { ps.erase(std::remove(ps.begin(), ps.end(), p), ps.end()); }
    ~Scratch() {
        (void)hipStreamSynchronize(st);
        for (void* p : ps) A.release(A.self, p);
    }
};

template <class T, class Op>
hipError_t scan_excl(Scratch& S, hipStream_t st, const T* in, T* out, size_t n, T* d_total) {
    const uint32_t nb = blocks(n, TILE);
    T* sums = S.get<T>(nb);
    if (!sums) return hipErrorOutOfMemory;
    k_scan_up<T, Op><<<nb, TB, 0, st>>>(in, n, sums);
    k_scan_mid<T, Op><<<1, TB, 0, st>>>(sums, nb, d_total);
    k_scan_down<T, Op><<<nb, TB, 0, st>>>(in, out, n, sums);
    return hipGetLastError();
}
// sorts (k[0], v[0]) by the low `bits` bits of the keys (stable); the result is left in (k[*which], v[*which])
hipError_t radix_sort(Scratch& S, hipStream_t st, uint32_t* k[2], uint32_t* v[2], size_t n, int bits, int* which) {
    const uint32_t nt = blocks(n, TILE);
    uint32_t* hist = S.get<uint32_t>((size_t)256 * nt);
    if (!hist) return hipErrorOutOfMemory;
    int cur = 0;
    for (int shift = 0; shift < std::max(bits, 1); shift += 8) {
        k_rs_hist<<<nt, TB, 0, st>>>(k[cur], n, shift, hist, nt);
        hipError_t e = scan_excl<uint32_t, SumU32>(S, st, hist, hist, (size_t)256 * nt, nullptr);
        if (e != hipSuccess) return e;
        k_rs_scatter<<<nt, TB, 0, st>>>(k[cur], v[cur], k[cur ^ 1], v[cur ^ 1], n, shift, hist, nt);
        cur ^= 1;
    }
    *which = cur;
    return hipGetLastError();
}

// step 3's launches: rounds until the frontier is empty, in batches between two looks at the round table.  *n_rounds: rounds launched.
// RV_OK, RV_COMPILE_FALLBACK (the cap: a chain of ops this deep compiles on the host) or RV_E_DEVICE.
struct RoundArgs {
    const rv_op* ops;
    const int2* prod;
    const uint32_t *uses, *cons_off, *cons;
    uint32_t* rem;
    int2* V;
    uint4* V3;
    int* glvl;
    uint32_t *mat, *frontier;
    uint2* rounds;
};
int run_rounds(hipStream_t st, int form, uint32_t chunk, size_t n, uint32_t max_rounds, const RoundArgs& a, uint32_t* n_rounds) {
    const uint32_t round_blocks = std::min<uint32_t>(blocks(n, TB), 1024);
    uint32_t r = 0, batch = 8;
    for (;;) {
        if (r >= max_rounds) return RV_COMPILE_FALLBACK;
        const uint32_t e = std::min(r + batch, max_rounds);
        for (; r < e; r++) {
#define CD_ROUND(F) k_cd_round<F><<<round_blocks, TB, 0, st>>>(r, chunk, a.ops, a.prod, a.uses, a.cons_off, a.cons, a.rem, a.V, a.V3, a.glvl, a.mat, a.frontier, a.rounds)
            if (form == FORM_LAZY) CD_ROUND(FORM_LAZY);
            else if (form == FORM_Z64) CD_ROUND(FORM_Z64);
            else CD_ROUND(FORM_K1);
#undef CD_ROUND
        }
        uint2 nxt;
        if (hipGetLastError() != hipSuccess || hipMemcpyAsync(&nxt, a.rounds + r, sizeof nxt, hipMemcpyDeviceToHost, st) != hipSuccess ||
            hipStreamSynchronize(st) != hipSuccess) {
            (void)hipGetLastError();
            return RV_E_DEVICE;
        }
        if (nxt.y == 0) {
            *n_rounds = r;
            return nxt.x == n ? RV_OK : RV_COMPILE_FALLBACK;  // (every op resolves exactly once; the second cannot happen)
        }
        batch = std::min<uint32_t>(batch * 2, 256);
    }
}

// What the Z64 side of a mixed list tells the GF(2) compile (compile_mixed_device): the ops are the list's GF(2) ops in order
struct Mixed {
    const uint32_t* orig;  // op i's place in the whole list (the AssertZero table)
    size_t n_total;        // ops of the whole list
    // The Z64 ops' writers and levels, run once the GF(2) ops have theirs (glvl2: the level of every GF(2) op's gate) -- a B2A gate
    // sits one level above its deepest reconstruction.  Fills levels64 and wb64; RV_OK or what the compile returns.
    std::function<int(const int* glvl2)> z64_levels;
    uint32_t levels64 = 0;  // levels the Z64 ops take (the level count is the deeper domain's, Builder::max_level)
    bool wb64 = false;      // a chunk whose Z64 side has write-back gates: they share the GF(2) write-backs' level
    // B2A expansions in the list (RV_COMPILE_DEVICE_B2A): where each starts, ascending, and what its Gate64 needs from this compile
    // (b2a_rows[2 j] = its first reconstruction's computed row, [2 j + 1] = its first fresh mask's row)
    uint32_t n_b2a = 0;
    const uint32_t* b2a_base = nullptr;
    uint32_t* b2a_rows = nullptr;
};
// Gate64::a and Gate64::m2 of every B2A (run_pass: first_out and m2_first, as share rows)
__global__ __launch_bounds__(TB) void k_cd_b2a_rows(const uint32_t* b2a_base, uint32_t n_b2a, const C4* cx, const uint32_t* comp, Seeds s, uint32_t pad,
                                                    uint32_t* rows) {
    const uint32_t j = blockIdx.x * TB + threadIdx.x;
    if (j >= n_b2a) return;
    const uint32_t b = b2a_base[j];
    rows[2 * j] = s.base + pad + 1 + comp[b + B2A_RECON0];
    rows[2 * j + 1] = s.base + s.m0 + cx[b].m;
}

int compile_gf2_device(hipStream_t st, const DevAlloc& A, const rv_op* d_ops, size_t n_ops, size_t z64_wires, size_t gf2_wires, bool keep_wires,
                       int force_lazy_k, Compiled& out, DevCompileKeep* keep, DevCompileLaps* laps, const ChunkStart* chunk, Mixed* mx) {
    // (a Z64 op in the list is what sends a program to the host; the Z64 wire count alone does not)
    const bool lazy = force_lazy_k == RV_LIN_K;  // the lazy-sum form: whole programs only (a chunk is final at K = 1)
    if (keep_wires || (force_lazy_k && (!lazy || chunk)) || getenv("RV_LAZY_K") || (n_ops == 0 && !chunk && !mx) || n_ops >= (1u << 28) || gf2_wires >= (1u << 31) ||
        (chunk && gf2_wires >= (1u << 30)))  // (a chunk names wire w's carried row -2 - w, below the host compiler's CARRY flag bit)
        return RV_COMPILE_FALLBACK;
    const size_t n = n_ops;
    const uint32_t W = (uint32_t)gf2_wires;
    const uint64_t LIM = 0xFFFFFFFFull - 512;
    Seeds seeds{0, 0, 0, 0, 0, 0};
    if (chunk) {
        if (chunk->mask_phase >= 128 || chunk->on0 > LIM || chunk->pre0 > LIM || z64_wires > LIM) return RV_COMPILE_FALLBACK;
        seeds.chunk = 1;
        seeds.base = W;
        seeds.m0 = chunk->mask_phase;
        seeds.on0 = (uint32_t)chunk->on0;
        seeds.pre0 = (uint32_t)chunk->pre0;
    }
    Scratch S(A, st);
    hipEvent_t ev[6] = {};
    const bool timed = laps != nullptr;
    if (timed)
        for (auto& e : ev)
            if (hipEventCreate(&e) != hipSuccess) return RV_E_DEVICE;
    struct EvGuard {
        hipEvent_t* e;
        ~EvGuard() {
            for (int k = 0; k < 6; k++)
                if (e[k]) (void)hipEventDestroy(e[k]);
        }
    } ev_guard{ev};
    auto mark = [&](int k) {
        if (timed) (void)hipEventRecord(ev[k], st);
    };
#define CDCHK(x)                                               \
    do {                                                       \
        if ((x) != hipSuccess) {                               \
            (void)hipGetLastError();                           \
            return S.failed ? RV_E_NOMEM : RV_E_DEVICE;        \
        }                                                      \
    } while (0)
#define CDNEED(p) \
    if (!(p)) return RV_E_NOMEM
    const uint32_t gb = blocks(n, TB);
    mark(0);
    // ---- 1. classify ----
    C4* cx = S.get<C4>(n + 1);
    uint32_t* kbuf[2] = {S.get<uint32_t>(n), S.get<uint32_t>(n)};
    uint32_t* vbuf[2] = {S.get<uint32_t>(n), S.get<uint32_t>(n)};
    uint32_t* d_small = S.get<uint32_t>(64);  // [0] error flag, [8..12) C4 totals, [16..24) DevStats, [24..28) the write-back totals
    CDNEED(cx && kbuf[0] && kbuf[1] && vbuf[0] && vbuf[1] && d_small);
    C4* d_tot = (C4*)(d_small + 8);
    DevStats* d_stats = (DevStats*)(d_small + 16);
    CDCHK(hipMemsetAsync(d_small, 0, 64 * 4, st));
    const uint32_t n_b2a = mx ? mx->n_b2a : 0, n_recon = 64u * n_b2a;  // (n_b2a x 442 < 2^28)
    k_cd_classify<<<gb, TB, 0, st>>>(d_ops, n, W, n_b2a ? 1u : 0u, cx, kbuf[0], vbuf[0], d_small);
    CDCHK(hipGetLastError());
    CDCHK((scan_excl<C4, SumC4>(S, st, cx, cx, n, d_tot)));
    uint32_t h_small[28];
    CDCHK(hipMemcpyAsync(h_small, d_small, sizeof h_small, hipMemcpyDeviceToHost, st));
    CDCHK(hipStreamSynchronize(st));
    if (h_small[0]) return RV_COMPILE_FALLBACK;  // an op the device path does not take, or an op-list error: the host compiler reports it
    const C4 tot{h_small[8], h_small[9], h_small[10], h_small[11]};
    const uint64_t n_on = (uint64_t)tot.in + tot.mul + tot.as, n_rec = (uint64_t)tot.mul + tot.as;
    uint32_t* rec_rows = nullptr;
    uint32_t* in_rows = nullptr;
    {
        void* p = nullptr;
        if (A.alloc(A.self, std::max<size_t>(n_rec, 1) * 4, &p) != RV_OK) return RV_E_NOMEM;
        rec_rows = (uint32_t*)p;
        S.ps.push_back(p);
        if (A.alloc(A.self, std::max<size_t>(tot.in, 1) * 4, &p) != RV_OK) return RV_E_NOMEM;
        in_rows = (uint32_t*)p;
        S.ps.push_back(p);
    }
    if (tot.as < n_recon) return RV_E_DEVICE;  // (cannot happen: every expansion has its 64 reconstructions)
    const uint32_t n_as = tot.as - n_recon;    // the AssertZero ops (a B2A's reconstructions count in tot.as, as in info.gf2_asserts)
    uint32_t* as_rec = S.get<uint32_t>(n_as);
    uint64_t* as_op = S.get<uint64_t>(n_as);
    CDNEED(as_rec && as_op);
    k_cd_ordinals<<<gb, TB, 0, st>>>(d_ops, n, cx, seeds.on0, rec_rows, in_rows, as_rec, as_op, mx ? mx->orig : nullptr, mx ? mx->b2a_base : nullptr, n_b2a);
    CDCHK(hipGetLastError());
    mark(1);
    // ---- 2. the last writer of every read ----
    int which = 0;
    CDCHK(radix_sort(S, st, kbuf, vbuf, n, bit_len(W), &which));
    uint32_t* seg_lo = S.get<uint32_t>(W);
    uint32_t* seg_hi = S.get<uint32_t>(W);
    int2* prod = S.get<int2>(n);
    uint32_t* uses = S.get<uint32_t>(n + 1);
    uint32_t* rem = S.get<uint32_t>(n);
    CDNEED(seg_lo && seg_hi && prod && uses && rem);
    CDCHK(hipMemsetAsync(seg_lo, 0, std::max<size_t>(W, 1) * 4, st));
    CDCHK(hipMemsetAsync(seg_hi, 0, std::max<size_t>(W, 1) * 4, st));
    CDCHK(hipMemsetAsync(uses, 0, (n + 1) * 4, st));
    k_cd_segs<<<gb, TB, 0, st>>>(kbuf[which], n, W, seg_lo, seg_hi);
    k_cd_resolve<<<gb, TB, 0, st>>>(d_ops, n, vbuf[which], seg_lo, seg_hi, seeds.chunk, prod, uses, rem);
    CDCHK(hipGetLastError());
    uint32_t* cons_off = S.get<uint32_t>(n + 1);
    uint32_t* cursor = S.get<uint32_t>(n);
    uint32_t* cons = S.get<uint32_t>(2 * n);
    CDNEED(cons_off && cursor && cons);
    CDCHK((scan_excl<uint32_t, SumU32>(S, st, uses, cons_off, n + 1, nullptr)));
    CDCHK(hipMemsetAsync(cursor, 0, n * 4, st));
    k_cd_consumers<<<gb, TB, 0, st>>>(prod, n, cons_off, cursor, cons);
    CDCHK(hipGetLastError());
    mark(2);
    // ---- 3. values and levels, round by round ----
    int2* V = lazy ? nullptr : S.get<int2>(n);
    uint4* V3 = lazy ? S.get<uint4>(n) : nullptr;
    int* glvl = S.get<int>(n);
    uint32_t* mat = S.get<uint32_t>(n + 1);
    uint32_t* frontier = S.get<uint32_t>(n);
    const uint32_t max_rounds = (uint32_t)std::min<size_t>(n + 1, MAX_ROUNDS);
    uint2* rounds = S.get<uint2>((size_t)max_rounds + 2);
    CDNEED((V || V3) && glvl && mat && frontier && rounds);
    CDCHK(hipMemsetAsync(rounds, 0, ((size_t)max_rounds + 2) * sizeof(uint2), st));
    CDCHK(hipMemsetAsync(mat + n, 0, 4, st));
    k_cd_front0<<<gb, TB, 0, st>>>(rem, n, frontier, rounds);
    CDCHK(hipGetLastError());
    uint32_t r = 0;
    {
        const RoundArgs ra{d_ops, prod, uses, cons_off, cons, rem, V, V3, glvl, mat, frontier, rounds};
        const int rr = run_rounds(st, lazy ? FORM_LAZY : FORM_K1, lazy ? 0u : seeds.chunk, n, max_rounds, ra, &r);
        if (rr != RV_OK) return rr;
    }
    if (laps) laps->rounds = r;
    if (mx && mx->z64_levels) {
        const int rz = mx->z64_levels(glvl);
        if (rz != RV_OK) return rz;
    }
    if (lazy) k_cd_stats<true><<<gb, TB, 0, st>>>(d_ops, n, prod, V, V3, glvl, mat, d_stats);
    else k_cd_stats<false><<<gb, TB, 0, st>>>(d_ops, n, prod, V, V3, glvl, mat, d_stats);
    CDCHK(hipGetLastError());
    // ---- 6a. (chunk mode) the wires the piece wrote, while the writers sort is still in place ----
    C4* wfl = nullptr;
    uint32_t* lastw = nullptr;
    if (chunk) {
        wfl = S.get<C4>(W);
        lastw = S.get<uint32_t>(W);
        CDNEED(wfl && lastw);
        k_cd_wb_flags<<<blocks(W, TB), TB, 0, st>>>(vbuf[which], seg_lo, seg_hi, W, V, wfl, lastw);
        CDCHK(hipGetLastError());
        CDCHK((scan_excl<C4, SumC4>(S, st, wfl, wfl, W, (C4*)(d_small + 24))));
    }
    // d_stats->max_level starts at 0 (memset): max_level + 1 levels when there are gates
    CDCHK(hipMemcpyAsync(h_small, d_small, sizeof h_small, hipMemcpyDeviceToHost, st));
    CDCHK(hipStreamSynchronize(st));
    DevStats hs;
    memcpy(&hs, h_small + 16, sizeof hs);
    mark(3);
    const uint64_t n_gates_ops = hs.n_gates;
    const uint32_t n_levels_ops = n_gates_ops ? (uint32_t)hs.max_level + 1 : 0;
    // the write-back level: one G_XORK per written wire behind every other level; the carried forms it reads are level 0's
    const uint32_t n_wb = chunk ? h_small[24] : 0, n_wbmat = chunk ? h_small[25] : 0, n_wbrow = chunk ? h_small[26] : 0;
    seeds.n_wbmat = n_wbmat;
    // (a mixed list: the deeper domain's levels count, and either domain's write-backs make the last level)
    const uint32_t levels64 = mx ? mx->levels64 : 0;
    const uint32_t wb_level = std::max<uint32_t>({n_levels_ops, n_wbmat ? 1u : 0u, levels64});
    const uint32_t n_levels = (n_wb || (mx && mx->wb64)) ? wb_level + 1 : std::max(n_levels_ops, levels64);
    const uint64_t n_gates = n_gates_ops + n_wbmat + n_wb;
    // the K = 1 compile is final unless the circuit is deep and narrow (compile_ops_seq): those go to the host compiler
    // (a chunk is compiled once, at K = 1, whatever its shape; a forced lazy-sum compile is final too)
    if (!chunk && !lazy && n_levels && lazy_forms_pay(n_levels, n_gates)) return RV_COMPILE_FALLBACK;
    const uint64_t n_masks = (uint64_t)seeds.m0 + tot.m;
    const uint64_t n_masks_pad = (n_masks + 127) / 128 * 128;
    const uint64_t n_comp = 1 + (uint64_t)hs.n_mat + n_wbmat;
    if ((uint64_t)W + n_masks_pad + n_comp > LIM || n_masks_pad / 128 > RV_MAX_CTR_BLOCKS || (uint64_t)n_levels * 5 + 1 >= (1ull << 32) ||
        n_comp > LIM / 2 || 1 + (uint64_t)W + n > LIM || (uint64_t)seeds.on0 + n_on > LIM || (uint64_t)seeds.pre0 + tot.mul > LIM)
        return RV_COMPILE_FALLBACK;
    // ---- 4. computed rows ----
    uint32_t* comp = S.get<uint32_t>(n + 1);
    CDNEED(comp);
    CDCHK((scan_excl<uint32_t, SumU32>(S, st, mat, comp, n + 1, nullptr)));
    if (n_b2a) {
        k_cd_b2a_rows<<<blocks(n_b2a, TB), TB, 0, st>>>(mx->b2a_base, n_b2a, cx, comp, seeds, (uint32_t)n_masks_pad, mx->b2a_rows);
        CDCHK(hipGetLastError());
    }
    // ---- 5. tables ----
    const uint32_t n_buckets = n_levels_ops * 5;  // (of the ops' gates: the write-back gates do not go through the sort)
    if (lazy) k_cd_keys<true><<<gb, TB, 0, st>>>(d_ops, n, prod, V, V3, glvl, mat, n_buckets, kbuf[0], vbuf[0]);
    else k_cd_keys<false><<<gb, TB, 0, st>>>(d_ops, n, prod, V, V3, glvl, mat, n_buckets, kbuf[0], vbuf[0]);
    CDCHK(hipGetLastError());
    CDCHK(radix_sort(S, st, kbuf, vbuf, n, bit_len(n_buckets), &which));
    void* pg = nullptr;
    if (A.alloc(A.self, std::max<size_t>(n_gates, 1) * sizeof(Gate), &pg) != RV_OK) return RV_E_NOMEM;
    S.ps.push_back(pg);
    Gate* gates = (Gate*)pg;
    uint32_t* pos = S.get<uint32_t>((size_t)n_buckets + 1);
    uint32_t* need_raw = S.get<uint32_t>(n_levels);
    uint32_t* on_lvl = S.get<uint32_t>(n_on + 1);
    uint32_t* pm = S.get<uint32_t>(n_on + 1);
    uint32_t* done_on = S.get<uint32_t>(n_levels);
    CDNEED(pos && need_raw && on_lvl && pm && done_on);
    CDCHK(hipMemsetAsync(need_raw, 0, std::max<size_t>(n_levels, 1) * 4, st));
    CDCHK(hipMemsetAsync(on_lvl + n_on, 0, 4, st));
    k_cd_bounds<<<blocks(n_gates_ops + 1, TB), TB, 0, st>>>(kbuf[which], n_gates_ops, n_buckets, pos);
    if (n_gates_ops && lazy)
        k_cd_gates<true><<<blocks(n_gates_ops, TB), TB, 0, st>>>(kbuf[which], vbuf[which], n_gates_ops, d_ops, prod, V, V3, cx, comp, seeds,
                                                                 (uint32_t)n_masks_pad, gates, need_raw, on_lvl);
    else if (n_gates_ops)
        k_cd_gates<false><<<blocks(n_gates_ops, TB), TB, 0, st>>>(kbuf[which], vbuf[which], n_gates_ops, d_ops, prod, V, V3, cx, comp, seeds,
                                                                  (uint32_t)n_masks_pad, gates, need_raw, on_lvl);
    if (n_wb)
        k_cd_wb_gates<<<blocks(W, TB), TB, 0, st>>>(lastw, wfl, W, d_ops, V, cx, comp, seeds, (uint32_t)n_masks_pad, hs.n_mat, n_buckets >= 3 ? pos + 3 : nullptr,
                                                    (uint32_t)(n_gates_ops + n_wbmat), gates);
    CDCHK(hipGetLastError());
    CDCHK((scan_excl<uint32_t, MaxU32>(S, st, on_lvl, pm, n_on + 1, nullptr)));
    k_cd_done_on<<<blocks(n_on + 1, TB), TB, 0, st>>>(pm, on_lvl, n_on, n_levels, done_on);
    CDCHK(hipGetLastError());
    mark(4);
    // ---- the host's copy (the planners of circuit_upload read it) ----
    Compiled& cc = out;
    cc = Compiled();
    cc.gates.resize(n_gates);
    cc.rec_rows.resize(n_rec);
    cc.in_rows.resize(tot.in);
    cc.assert_rec2.resize(n_as);
    cc.assert_op2.resize(n_as);
    std::vector<uint32_t> h_pos((size_t)n_buckets + 1), h_need(n_levels);
    cc.level_done_on.resize(n_levels);
    auto d2h = [&](void* dst, const void* src, size_t bytes) { return bytes ? hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, st) : hipSuccess; };
    CDCHK(d2h(cc.gates.data(), gates, n_gates * sizeof(Gate)));
    CDCHK(d2h(cc.rec_rows.data(), rec_rows, n_rec * 4));
    CDCHK(d2h(cc.in_rows.data(), in_rows, (size_t)tot.in * 4));
    CDCHK(d2h(cc.assert_rec2.data(), as_rec, (size_t)n_as * 4));
    CDCHK(d2h(cc.assert_op2.data(), as_op, (size_t)n_as * 8));
    CDCHK(d2h(h_pos.data(), pos, h_pos.size() * 4));
    CDCHK(d2h(h_need.data(), need_raw, (size_t)n_levels * 4));
    CDCHK(d2h(cc.level_done_on.data(), done_on, (size_t)n_levels * 4));
    mark(5);
    CDCHK(hipStreamSynchronize(st));
    cc.level_start.assign(n_levels + 1, 0);
    cc.level_range.assign(n_levels, LevelRange{});
    cc.level_need_blocks.assign(n_levels, 0);
    uint32_t need = 0;
    // first gate with key >= k: the ops' gates (h_pos), the materialised carried forms (key 3) and the write-backs (the last level's key 3)
    auto first_at = [&](size_t k) {
        uint64_t v = k <= n_buckets ? h_pos[k] : n_gates_ops;
        if (k >= 4) v += n_wbmat;
        if (n_wb && k >= (size_t)wb_level * 5 + 4) v += n_wb;
        return (uint32_t)v;
    };
    for (uint32_t l = 0; l < n_levels; l++) {
        uint32_t e[6];
        for (int j = 0; j < 6; j++) e[j] = first_at((size_t)l * 5 + j);
        cc.level_start[l] = e[0];
        cc.level_range[l] = LevelRange{e[0], e[1], e[2], e[3], e[4], e[5]};
        need = std::max(need, h_need[l]);
        cc.level_need_blocks[l] = need;
        cc.level_done_on[l] += seeds.on0;  // (the carried rows in front are complete before level 0)
    }
    cc.level_start[n_levels] = (uint32_t)n_gates;
    cc.level_start64.assign(n_levels + 1, 0);
    const uint64_t randoms = (uint64_t)tot.m - tot.in - 2ull * tot.mul;
    cc.n_ssa = 1 + (chunk ? (uint64_t)W : 0) + n - n_as;
    cc.n_masks = n_masks;
    cc.n_masks_pad = n_masks_pad;
    cc.n_rows = (chunk ? (uint64_t)W : 0) + n_masks_pad + n_comp;
    cc.n_on = (chunk ? chunk->on0 : 0) + n_on;
    cc.n_pre = (chunk ? chunk->pre0 : 0) + tot.mul;
    cc.n_in = tot.in;
    cc.n_rec = n_rec;
    cc.n_random_or_recon = randoms + n_recon;
    cc.n_user_random = randoms - n_recon;  // (a B2A's 64 fresh masks are not the user's)
    cc.row_prg_base = chunk ? W : 0;
    cc.zero_row = cc.row_prg_base + n_masks_pad;
    if (chunk) {  // (the Z64 side of a GF(2) piece: its carried slots and counters, untouched)
        cc.n_ssa64 = 1 + z64_wires;
        cc.n_masks64 = chunk->mask64_phase;
        cc.on_words64 = chunk->on_words64_0;
        cc.pre_words64 = chunk->pre_words64_0;
    }
    rv_circuit_info& info = cc.info;
    info.n_ops = mx ? mx->n_total : n;
    info.gf2_inputs = tot.in;
    info.gf2_muls = tot.mul;
    info.gf2_asserts = tot.as;
    info.gf2_linear = randoms + (hs.n_mat - n_recon) + n_wbmat + n_wb;  // (n_mat: every gate with a computed row, reconstructions too)
    info.gf2_masks = n_masks;
    info.z64_masks = cc.n_masks64;
    info.levels = n_levels;
    info.gf2_operand_rows = hs.operand_rows + n_wbmat + n_wbrow;
    info.gf2_rows_written = (uint64_t)hs.n_mat + n_wbmat + n_wb;
    if (laps) {
        float ms[5] = {0, 0, 0, 0, 0};
        for (int k = 0; k < 5; k++) (void)hipEventElapsedTime(&ms[k], ev[k], ev[k + 1]);
        laps->classify = ms[0];
        laps->writers = ms[1];
        laps->levels = ms[2];
        laps->tables = ms[3];
        laps->download = ms[4];
    }
    if (keep) {
        keep->d_gates = gates;
        keep->d_rec_rows = rec_rows;
        keep->d_in_rows = in_rows;
        S.keep(gates);
        S.keep(rec_rows);
        S.keep(in_rows);
    }
    return RV_OK;
}

// ---- Z64 ops and mixed lists (RV_COMPILE_DEVICE_Z64) ----
// The two domains share no wire and, without B2A, no gate: run_pass keeps them apart except for the level count.  So a mixed list is
// split: its GF(2) ops, compacted in order, go through the pipeline above unchanged, and its Z64 ops through the same steps in a
// simpler form -- no folding, every op one Gate64, every counter a prefix sum, a gate's level one above its deepest operand.
// B2A (RV_COMPILE_DEVICE_B2A) is the one dependency between them, and it runs one way: a B2A is expanded at the split into its 442
// GF(2) steps (k_z_expand) and one Z64-list record; the GF(2) pipeline runs its levels first, the B2A records take theirs from their
// reconstructions' (k_z_b2a_levels), and the Z64 rounds start from there.
//   1. classify    one thread per op of the whole list: the Z64 and SizeHint checks of run_pass (the GF(2) ops are checked by
//                  k_cd_classify once compacted), the Z64 counters and each op's place in its domain's list: two 16-byte tuple scans
//   2. writers     the sort, segments and resolve kernels above, over the Z64 ops and wires
//   3. levels      the round kernel in its FORM_Z64
//   4. tables      a stable sort by level; the records, offsets and AssertZero tables written by one thread per gate; a chunk's
//                  write-back copies (one G64_ADDC per written wire, in wire order) behind them
static_assert(sizeof(Gate64) == 64, "Gate64 is compared bytewise: no padding");
struct Seeds64 {
    uint32_t ssa_base;  // the first op's SSA id: 1, or 1 + z64_wires behind a chunk's carried slots
    uint32_t m0;        // ShareGen<Z64> calls before the piece (mask64_phase)
    uint64_t on0, pre0;  // transcript words in front of the piece's own
};

// pc: {GF(2) op, Z64 op, 0, 0} -- their exclusive scan is every op's place in its domain's list; zc: the Z64 counters of compile.cpp
// (m: Input 1, Random 1, Mul 2; mul; as; in).  A B2A op, an unknown domain, a SizeHint that grows a wire count and any Z64 op
// run_pass rejects raise the flag: the host compiler takes the list.
// admit_b2a: a B2A op is {442 entries of the GF(2) list, one of the Z64 list, one B2A} in pc and one Z64 mask in zc, checked as
// run_pass checks it (dst in the Z64 wires, the 64 source wires in the GF(2) wires).
__global__ __launch_bounds__(TB) void k_z_classify(const rv_op* ops, size_t n, uint32_t W2, uint32_t W64, uint32_t admit_b2a, C4* zc, C4* pc, uint32_t* flag) {
    const size_t i = (size_t)blockIdx.x * TB + threadIdx.x;
    if (i >= n) return;
    const rv_op op = ops[i];
    bool bad = op.reserved != 0;
    C4 z{0, 0, 0, 0}, p{0, 0, 0, 0};
    if (op.domain == RV_DOM_GF2) {
        p.m = 1;
    } else if (op.domain == RV_DOM_Z64) {
        if (op.opcode > RV_OP_CONST) bad = true;
        const int nr = bad ? 0 : op_reads(op.opcode);
        if (!bad && op_writes(op.opcode) && op.dst >= W64) bad = true;
        if (nr >= 1 && op.a >= W64) bad = true;
        if (nr >= 2 && op.b >= W64) bad = true;
        p.mul = 1;
        if (op.opcode == RV_OP_INPUT) z.m = 1, z.in = 1;
        else if (op.opcode == RV_OP_RANDOM) z.m = 1;
        else if (op.opcode == RV_OP_MUL) z.m = 2, z.mul = 1;
        else if (op.opcode == RV_OP_ASSERTZERO) z.as = 1;
    } else if (op.domain == RV_DOM_SIZEHINT) {
        if (op.a > W64 || op.b > W2) bad = true;
    } else if (op.domain == RV_DOM_B2A && admit_b2a) {
        if (op.dst >= W64 || (uint64_t)op.a + 64 > W2) bad = true;
        p.m = B2A_STEPS, p.mul = 1, p.as = 1;
        z.m = 1;
    } else {
        bad = true;
    }
    if (bad) atomicOr(flag, 1u);
    zc[i] = z;
    pc[i] = p;
}
// px, zx: the exclusive scans.  Each domain's ops in order, with their places in the whole list; the Z64 ops' counters go with them
// A B2A goes into the Z64 list as a ZOP_B2A record whose `a` is the place of its expansion in the GF(2) list (k_z_expand fills that);
// bx64 (null: a list without B2A): the B2A ops in front of every Z64-list entry -- they share the correction ordinal with Mul;
// b2a: per B2A {its expansion's place, its first source wire, its place in the whole list}
__global__ __launch_bounds__(TB) void k_z_compact(const rv_op* ops, size_t n, const C4* px, const C4* zx, rv_op* ops2, uint32_t* orig2, rv_op* ops64,
                                                  uint32_t* orig64, C4* zc64, uint32_t* bx64, uint32_t* b2a_base, uint2* b2a_src) {
    const size_t i = (size_t)blockIdx.x * TB + threadIdx.x;
    if (i >= n) return;
    const rv_op op = ops[i];
    const C4 p = px[i];
    if (op.domain == RV_DOM_GF2) {
        ops2[p.m] = op;
        orig2[p.m] = (uint32_t)i;
    } else if (op.domain == RV_DOM_Z64 || op.domain == RV_DOM_B2A) {
        rv_op o = op;
        if (op.domain == RV_DOM_B2A) {
            o.domain = RV_DOM_Z64, o.opcode = ZOP_B2A, o.reserved = 0, o.a = p.m, o.b = 0, o.imm = 0;
            b2a_base[p.as] = p.m;
            b2a_src[p.as] = make_uint2(op.a, (uint32_t)i);
        }
        ops64[p.mul] = o;
        orig64[p.mul] = (uint32_t)i;
        zc64[p.mul] = zx[i];
        if (bx64) bx64[p.mul] = p.as;
    }
}
// Step j of a B2A's expansion (run_pass, case RV_DOM_B2A, in Builder::g_* call order) at place B of the GF(2) list, S = its first source
// wire: 64 Random a_k; Mul(a_0, b_0), Xor(a_0, b_0); for k = 1..62 ac = Xor(a_k, carry), bc = Xor(b_k, carry), t = Mul(ac, bc),
// res_k = Xor(ac, b_k), carry = Xor(t, carry); Xor(a_63, b_63), res_63 = Xor(carry, that); 64 reconstructions of res_k
__device__ inline rv_op b2a_step(uint32_t B, uint32_t S, uint32_t j) {
    rv_op o;
    o.domain = RV_DOM_GF2, o.opcode = RV_OP_ADD, o.reserved = PS_OP | PS_A | PS_B, o.dst = 0, o.a = 0, o.b = 0, o.imm = 0;
    if (j < 64) {
        o.opcode = RV_OP_RANDOM, o.reserved = PS_OP;
    } else if (j == 64 || j == 65) {
        o.opcode = j == 64 ? RV_OP_MUL : RV_OP_ADD;
        o.reserved = PS_OP | PS_A, o.a = B, o.b = S;
    } else if (j < 376) {
        const uint32_t k = 1 + (j - 66) / 5, t = (j - 66) % 5, at = 66 + 5 * (k - 1), carry = k == 1 ? 64u : at - 1;
        if (t == 0) o.a = B + k, o.b = B + carry;
        else if (t == 1) o.reserved = PS_OP | PS_B, o.a = S + k, o.b = B + carry;
        else if (t == 2) o.opcode = RV_OP_MUL, o.a = B + at, o.b = B + at + 1;
        else if (t == 3) o.reserved = PS_OP | PS_A, o.a = B + at, o.b = S + k;
        else o.a = B + at + 2, o.b = B + carry;
    } else if (j == 376) {
        o.reserved = PS_OP | PS_A, o.a = B + 63, o.b = S + 63;
    } else if (j == 377) {
        o.a = B + 375, o.b = B + 376;
    } else {
        const uint32_t k = j - B2A_RECON0;
        o.opcode = RV_OP_ASSERTZERO, o.reserved = PS_OP | PS_A;
        o.a = B + (k == 0 ? 65u : k == 63 ? 377u : 66 + 5 * (k - 1) + 3);
    }
    return o;
}
static_assert(66 + 5 * 62 == 376 && B2A_RECON0 + 64 == B2A_STEPS, "the steps of one B2A");
// one workgroup per B2A
__global__ __launch_bounds__(TB) void k_z_expand(const uint32_t* b2a_base, const uint2* b2a_src, rv_op* ops2, uint32_t* orig2) {
    const uint32_t B = b2a_base[blockIdx.x];
    const uint2 s = b2a_src[blockIdx.x];
    for (uint32_t j = threadIdx.x; j < B2A_STEPS; j += TB) {
        ops2[B + j] = b2a_step(B, s.x, j);
        orig2[B + j] = s.y;
    }
}
// a B2A gate's level, before the Z64 rounds: one above its deepest reconstruction (glvl2: the GF(2) list's gate levels)
__global__ __launch_bounds__(TB) void k_z_b2a_levels(const rv_op* ops64, size_t n, const int* glvl2, int* glvl) {
    const size_t i = (size_t)blockIdx.x * TB + threadIdx.x;
    if (i >= n) return;
    const rv_op op = ops64[i];
    if (op.opcode != ZOP_B2A) return;
    int l = 0;
    for (uint32_t k = 0; k < 64; k++) l = max(l, glvl2[op.a + B2A_RECON0 + k]);
    glvl[i] = l + 1;
}
// the writer sort's keys (as k_cd_classify's: the wire, W64 for AssertZero)
__global__ __launch_bounds__(TB) void k_z_wkeys(const rv_op* ops, size_t n, uint32_t W64, uint32_t* keys, uint32_t* vals) {
    const size_t i = (size_t)blockIdx.x * TB + threadIdx.x;
    if (i >= n) return;
    const rv_op op = ops[i];
    keys[i] = op_writes(op.opcode) ? op.dst : W64;
    vals[i] = (uint32_t)i;
}
// the level sort's keys, and the deepest level (one atomic per wavefront)
__global__ __launch_bounds__(TB) void k_z_lkeys(const int* glvl, size_t n, uint32_t* keys, uint32_t* vals, uint32_t* max_level) {
    const size_t i = (size_t)blockIdx.x * TB + threadIdx.x;
    const uint32_t l = i < n ? (uint32_t)glvl[i] : 0u;
    if (i < n) {
        keys[i] = l;
        vals[i] = (uint32_t)i;
    }
    const uint32_t m = wave_max_u32(l);
    if ((threadIdx.x & 63u) == 0 && m) atomicMax(max_level, m);
}
// a chunk's written wires (each gets a write-back: an op's SSA id is never the carried slot's)
__global__ __launch_bounds__(TB) void k_z_wb_flags(const uint32_t* seg_lo, const uint32_t* seg_hi, uint32_t W64, uint32_t* fl) {
    const size_t w = (size_t)blockIdx.x * TB + threadIdx.x;
    if (w >= W64) return;
    fl[w] = seg_hi[w] > seg_lo[w];
}
// an operand: its SSA id (never written: 0; a chunk's carried slot 1 + w) and where its mask row lives (Builder::emit64's ssa_row64)
__device__ inline uint32_t z_ssa(int p, const C4* zc, const Seeds64& s) {
    return p >= 0 ? s.ssa_base + (uint32_t)p - zc[p].as : p == -1 ? 0u : 1u + (uint32_t)(-2 - p);
}
__device__ inline uint32_t z_mask_row(int p, const rv_op* ops, const C4* zc, const Seeds64& s) {
    if (p >= 0) {
        const uint32_t opc = ops[p].opcode;
        if (opc == RV_OP_INPUT || opc == RV_OP_RANDOM) return G64_MASK_ROW | (s.m0 + zc[p].m);
        if (opc == RV_OP_MUL) return G64_MASK_ROW | (s.m0 + zc[p].m + 1);
    }
    return z_ssa(p, zc, s);
}
// the Gate64 records in (level, program) order; the input / reconstruction offsets and the AssertZero tables by ordinal
// (bx: the B2A ops in front of each op, null without any; b2a_rows: Mixed::b2a_rows)
__global__ __launch_bounds__(TB) void k_z_gates(const uint32_t* sv, size_t n, const rv_op* ops, const int2* prod, const C4* zc, const uint32_t* orig, Seeds64 s,
                                                const uint32_t* bx, const uint32_t* b2a_rows, Gate64* gates, uint64_t* rec_offs, uint64_t* in_offs,
                                                uint32_t* as_rec, uint64_t* as_op) {
    const size_t p = (size_t)blockIdx.x * TB + threadIdx.x;
    if (p >= n) return;
    const uint32_t i = sv[p];
    const rv_op op = ops[i];
    const C4 c = zc[i];
    const int2 pr = prod[i];
    const int nr = op_reads(op.opcode);
    Gate64 g;
    g.op = 0, g.dst = 0, g.a = 0, g.b = 0, g.m = 0, g.m2 = 0, g.eo = 0, g.ep = 0, g.x = 0, g.xc = 0;
    g.imm = op.imm;
    g.a = nr >= 1 ? z_ssa(pr.x, zc, s) : 0u;
    g.b = nr >= 2 ? z_ssa(pr.y, zc, s) : 0u;
    g.am = nr >= 1 ? z_mask_row(pr.x, ops, zc, s) : 0u;
    g.bm = nr >= 2 ? z_mask_row(pr.y, ops, zc, s) : 0u;
    if (op_writes(op.opcode)) g.dst = s.ssa_base + i - c.as;
    const uint64_t eo = s.on0 + c.in + 8ull * ((uint64_t)c.mul + c.as);
    const uint32_t x = c.mul + c.as;
    const uint32_t nb = bx ? bx[i] : 0u, corr = c.mul + nb;  // corrections so far: Mul and B2A
    switch (op.opcode) {
    case ZOP_B2A:
        g.op = G64_B2A;
        g.a = b2a_rows[2 * nb];
        g.m = s.m0 + c.m;
        g.m2 = b2a_rows[2 * nb + 1];
        g.ep = s.pre0 + corr;
        g.xc = corr;
        break;
    case RV_OP_INPUT:
        g.op = G64_INPUT;
        g.m = s.m0 + c.m;
        g.eo = eo;
        g.x = c.in;
        in_offs[c.in] = eo;
        break;
    case RV_OP_RANDOM:
        g.op = G64_RANDOM;
        g.m = s.m0 + c.m;
        break;
    case RV_OP_CONST: g.op = G64_CONST; break;
    case RV_OP_ADD: g.op = G64_ADD; break;
    case RV_OP_SUB: g.op = G64_SUB; break;
    case RV_OP_ADDCONST: g.op = G64_ADDC; break;
    case RV_OP_SUBCONST: g.op = G64_SUBC; break;
    case RV_OP_MULCONST: g.op = G64_MULC; break;
    case RV_OP_MUL:
        g.op = G64_MUL;
        g.m = s.m0 + c.m;
        g.ep = s.pre0 + corr;
        g.xc = corr;
        g.eo = eo;
        g.x = x;
        rec_offs[x] = eo;
        break;
    default:  // AssertZero
        g.op = G64_ASSERT;
        g.eo = eo;
        g.x = x;
        rec_offs[x] = eo;
        as_rec[c.as] = x;
        as_op[c.as] = orig ? orig[i] : i;
        break;
    }
    gates[p] = g;
}
// a chunk's write-back level: wire w's final value copied to its carried slot.  sv: the writer sort's op indices; fx: the exclusive
// scan of k_z_wb_flags
__global__ __launch_bounds__(TB) void k_z_wb_gates(const uint32_t* sv, const uint32_t* seg_lo, const uint32_t* seg_hi, const uint32_t* fx, uint32_t W64,
                                                   const rv_op* ops, const C4* zc, Seeds64 s, Gate64* gates) {
    const size_t w = (size_t)blockIdx.x * TB + threadIdx.x;
    if (w >= W64 || seg_hi[w] <= seg_lo[w]) return;
    const int q = (int)sv[seg_hi[w] - 1];
    Gate64 g;
    g.op = G64_ADDC, g.dst = 1u + (uint32_t)w, g.b = 0, g.m = 0, g.m2 = 0, g.eo = 0, g.ep = 0, g.x = 0, g.xc = 0, g.imm = 0, g.bm = 0;
    g.a = z_ssa(q, zc, s);
    g.am = z_mask_row(q, ops, zc, s);
    gates[fx[w]] = g;
}

int compile_mixed_device(hipStream_t st, const DevAlloc& A, const rv_op* d_ops, size_t n, size_t z64_wires, size_t gf2_wires, bool keep_wires, int force_lazy_k,
                         Compiled& out, DevCompileKeep* keep, DevCompileLaps* laps, const ChunkStart* chunk, bool admit_b2a) {
    const bool lazy = force_lazy_k == RV_LIN_K;
    if (keep_wires || (force_lazy_k && (!lazy || chunk)) || getenv("RV_LAZY_K") || n >= (1u << 28) || gf2_wires >= (1u << 31) || z64_wires >= (1u << 30))
        return RV_COMPILE_FALLBACK;
    if (n == 0)  // (an empty piece; an empty program is the host compiler's)
        return compile_gf2_device(st, A, d_ops, n, z64_wires, gf2_wires, keep_wires, force_lazy_k, out, keep, laps, chunk, nullptr);
    const uint32_t W2 = (uint32_t)gf2_wires, W64 = (uint32_t)z64_wires;
    const uint64_t LIM = 0xFFFFFFFFull - 512;
    if (chunk && (chunk->mask64_phase >= 2 || chunk->on_words64_0 > (1ull << 62) || chunk->pre_words64_0 > (1ull << 62))) return RV_COMPILE_FALLBACK;
    Scratch S(A, st);
    hipEvent_t ev[6] = {};  // the split [0, 1), the Z64 tables [2, 3), the Z64 levels inside the GF(2) compile [4, 5)
    if (laps)
        for (auto& e : ev)
            if (hipEventCreate(&e) != hipSuccess) return RV_E_DEVICE;
    struct EvGuard {
        hipEvent_t* e;
        ~EvGuard() {
            for (int k = 0; k < 6; k++)
                if (e[k]) (void)hipEventDestroy(e[k]);
        }
    } ev_guard{ev};
    auto mark = [&](int k) {
        if (laps) (void)hipEventRecord(ev[k], st);
    };
    const uint32_t gb = blocks(n, TB);
    mark(0);
    // ---- 1. classify, split ----
    C4* zx = S.get<C4>(n);
    C4* px = S.get<C4>(n);
    uint32_t* d_small = S.get<uint32_t>(32);  // [0] error flag, [4..8) Z64 counter totals, [8..12) op counts, [12] deepest Z64 level, [13] write-backs
    CDNEED(zx && px && d_small);
    CDCHK(hipMemsetAsync(d_small, 0, 32 * 4, st));
    k_z_classify<<<gb, TB, 0, st>>>(d_ops, n, W2, W64, admit_b2a ? 1u : 0u, zx, px, d_small);
    CDCHK(hipGetLastError());
    CDCHK((scan_excl<C4, SumC4>(S, st, zx, zx, n, (C4*)(d_small + 4))));
    CDCHK((scan_excl<C4, SumC4>(S, st, px, px, n, (C4*)(d_small + 8))));
    uint32_t h_small[16];
    CDCHK(hipMemcpyAsync(h_small, d_small, sizeof h_small, hipMemcpyDeviceToHost, st));
    CDCHK(hipStreamSynchronize(st));
    if (h_small[0]) return RV_COMPILE_FALLBACK;
    const C4 tot{h_small[4], h_small[5], h_small[6], h_small[7]};
    const uint32_t n_b2a = h_small[10];
    if ((uint64_t)n_b2a * B2A_STEPS >= (1u << 28)) return RV_COMPILE_FALLBACK;  // (the expanded GF(2) list: below 2^28 entries, and no sum above wrapped)
    const size_t n2 = h_small[8], n64 = h_small[9];
    if (n2 == n && n64 == 0)  // no Z64 op, no B2A and no SizeHint: the list as it is
        return compile_gf2_device(st, A, d_ops, n, z64_wires, gf2_wires, keep_wires, force_lazy_k, out, keep, laps, chunk, nullptr);
    Seeds64 s64{1u + (chunk ? W64 : 0u), chunk ? chunk->mask64_phase : 0u, chunk ? chunk->on_words64_0 : 0, chunk ? chunk->pre_words64_0 : 0};
    const uint64_t n_masks64 = (uint64_t)s64.m0 + tot.m;
    if ((uint64_t)s64.ssa_base + n64 > LIM || n_masks64 > LIM || (n_masks64 + 1) / 2 > RV_MAX_CTR_BLOCKS) return RV_COMPILE_FALLBACK;
    rv_op* ops2 = S.get<rv_op>(n2);
    uint32_t* orig2 = S.get<uint32_t>(n2);
    rv_op* ops64 = S.get<rv_op>(n64);
    uint32_t* orig64 = S.get<uint32_t>(n64);
    C4* zc = S.get<C4>(n64);
    CDNEED(ops2 && orig2 && ops64 && orig64 && zc);
    uint32_t *bx64 = nullptr, *b2a_base = nullptr, *b2a_rows = nullptr;
    uint2* b2a_src = nullptr;
    if (n_b2a) {
        bx64 = S.get<uint32_t>(n64);
        b2a_base = S.get<uint32_t>(n_b2a);
        b2a_src = S.get<uint2>(n_b2a);
        b2a_rows = S.get<uint32_t>(2 * (size_t)n_b2a);
        CDNEED(bx64 && b2a_base && b2a_src && b2a_rows);
    }
    k_z_compact<<<gb, TB, 0, st>>>(d_ops, n, px, zx, ops2, orig2, ops64, orig64, zc, bx64, b2a_base, b2a_src);
    if (n_b2a) k_z_expand<<<n_b2a, TB, 0, st>>>(b2a_base, b2a_src, ops2, orig2);
    CDCHK(hipGetLastError());
    mark(1);
    // ---- 2. / 3. the Z64 ops' writers and levels: once the GF(2) ops have theirs (Mixed::z64_levels) ----
    const uint32_t gb64 = blocks(n64, TB);
    uint32_t *kbuf[2] = {nullptr, nullptr}, *vbuf[2] = {nullptr, nullptr}, *seg_lo = nullptr, *seg_hi = nullptr, *wbx = nullptr;
    int2* prod = nullptr;
    int* glvl = nullptr;
    int wsort = 0;
    uint32_t levels64 = 0, n_wb64 = 0;
    uint32_t *lk[2] = {nullptr, nullptr}, *lv[2] = {nullptr, nullptr};
    Mixed mx;
    mx.orig = orig2, mx.n_total = n;
    mx.n_b2a = n_b2a, mx.b2a_base = b2a_base, mx.b2a_rows = b2a_rows;
    mx.z64_levels = [&](const int* glvl2) -> int {
        if (!n64) return RV_OK;
        mark(4);
        for (int k = 0; k < 2; k++) kbuf[k] = S.get<uint32_t>(n64), vbuf[k] = S.get<uint32_t>(n64);
        seg_lo = S.get<uint32_t>(W64);
        seg_hi = S.get<uint32_t>(W64);
        prod = S.get<int2>(n64);
        uint32_t* uses = S.get<uint32_t>(n64 + 1);
        uint32_t* rem = S.get<uint32_t>(n64);
        uint32_t* cons_off = S.get<uint32_t>(n64 + 1);
        uint32_t* cursor = S.get<uint32_t>(n64);
        uint32_t* cons = S.get<uint32_t>(2 * n64);
        glvl = S.get<int>(n64);
        uint32_t* frontier = S.get<uint32_t>(n64);
        const uint32_t max_rounds = (uint32_t)std::min<size_t>(n64 + 1, MAX_ROUNDS);
        uint2* rounds = S.get<uint2>((size_t)max_rounds + 2);
        CDNEED(kbuf[0] && kbuf[1] && vbuf[0] && vbuf[1] && seg_lo && seg_hi && prod && uses && rem && cons_off && cursor && cons && glvl && frontier && rounds);
        k_z_wkeys<<<gb64, TB, 0, st>>>(ops64, n64, W64, kbuf[0], vbuf[0]);
        CDCHK(hipGetLastError());
        CDCHK(radix_sort(S, st, kbuf, vbuf, n64, bit_len(W64), &wsort));
        CDCHK(hipMemsetAsync(seg_lo, 0, std::max<size_t>(W64, 1) * 4, st));
        CDCHK(hipMemsetAsync(seg_hi, 0, std::max<size_t>(W64, 1) * 4, st));
        CDCHK(hipMemsetAsync(uses, 0, (n64 + 1) * 4, st));
        k_cd_segs<<<gb64, TB, 0, st>>>(kbuf[wsort], n64, W64, seg_lo, seg_hi);
        k_cd_resolve<<<gb64, TB, 0, st>>>(ops64, n64, vbuf[wsort], seg_lo, seg_hi, chunk ? 1u : 0u, prod, uses, rem);
        CDCHK(hipGetLastError());
        CDCHK((scan_excl<uint32_t, SumU32>(S, st, uses, cons_off, n64 + 1, nullptr)));
        CDCHK(hipMemsetAsync(cursor, 0, n64 * 4, st));
        CDCHK(hipMemsetAsync(rounds, 0, ((size_t)max_rounds + 2) * sizeof(uint2), st));
        k_cd_consumers<<<gb64, TB, 0, st>>>(prod, n64, cons_off, cursor, cons);
        k_cd_front0<<<gb64, TB, 0, st>>>(rem, n64, frontier, rounds);
        if (n_b2a) k_z_b2a_levels<<<gb64, TB, 0, st>>>(ops64, n64, glvl2, glvl);
        CDCHK(hipGetLastError());
        uint32_t r = 0;
        const RoundArgs ra{ops64, prod, uses, cons_off, cons, rem, nullptr, nullptr, glvl, nullptr, frontier, rounds};
        const int rr = run_rounds(st, FORM_Z64, 0u, n64, max_rounds, ra, &r);
        if (rr != RV_OK) return rr;
        if (chunk) {
            wbx = S.get<uint32_t>(W64);
            CDNEED(wbx);
            k_z_wb_flags<<<blocks(W64, TB), TB, 0, st>>>(seg_lo, seg_hi, W64, wbx);
            CDCHK(hipGetLastError());
            CDCHK((scan_excl<uint32_t, SumU32>(S, st, wbx, wbx, W64, d_small + 13)));
        }
        // the level sort's keys (the writer sort's values stay in vbuf[wsort] for the write-back gates; its other three buffers are free)
        lk[0] = kbuf[wsort], lk[1] = kbuf[wsort ^ 1];
        lv[0] = vbuf[wsort ^ 1], lv[1] = S.get<uint32_t>(n64);
        CDNEED(lv[1]);
        k_z_lkeys<<<gb64, TB, 0, st>>>(glvl, n64, lk[0], lv[0], d_small + 12);
        CDCHK(hipGetLastError());
        CDCHK(hipMemcpyAsync(h_small, d_small, sizeof h_small, hipMemcpyDeviceToHost, st));
        CDCHK(hipStreamSynchronize(st));
        levels64 = h_small[12] + 1;
        n_wb64 = chunk ? h_small[13] : 0;
        mx.levels64 = levels64, mx.wb64 = n_wb64 != 0;
        mark(5);
        return RV_OK;
    };
    // ---- the GF(2) ops (a B2A's 442 steps among them) ----
    {
        const int rc = compile_gf2_device(st, A, ops2, n2, z64_wires, gf2_wires, keep_wires, force_lazy_k, out, keep, laps, chunk, &mx);
        if (rc != RV_OK) return rc;
    }
    Compiled& cc = out;
    // (from here on a failure gives back what the GF(2) compile kept for the circuit)
    struct KeepGuard {
        const DevAlloc& A;
        hipStream_t st;
        DevCompileKeep* k;
        bool ok = false;
        ~KeepGuard() {
            if (ok || !k) return;
            (void)hipStreamSynchronize(st);
            for (void* p : {(void*)k->d_gates, (void*)k->d_rec_rows, (void*)k->d_in_rows, (void*)k->d_gates64, (void*)k->d_rec_offs64, (void*)k->d_in_offs64})
                if (p) A.release(A.self, p);
            *k = DevCompileKeep();
        }
    } keep_guard{A, st, keep};
    const uint32_t n_levels = (uint32_t)cc.level_start.size() - 1;
    cc.level_start64.assign((size_t)n_levels + 1, 0);
    if (n64) {
        if (n_levels < levels64 + (n_wb64 ? 1u : 0u)) return RV_E_DEVICE;  // (cannot happen)
        mark(2);
        // ---- 4. the Z64 tables ----
        const uint64_t n_rec64 = (uint64_t)tot.mul + tot.as, n_g64 = (uint64_t)n64 + n_wb64;
        Gate64* gates64 = nullptr;
        uint64_t *rec_offs = nullptr, *in_offs = nullptr;
        {
            void* p = nullptr;
            if (A.alloc(A.self, n_g64 * sizeof(Gate64), &p) != RV_OK) return RV_E_NOMEM;
            S.ps.push_back(p), gates64 = (Gate64*)p;
            if (A.alloc(A.self, std::max<uint64_t>(n_rec64, 1) * 8, &p) != RV_OK) return RV_E_NOMEM;
            S.ps.push_back(p), rec_offs = (uint64_t*)p;
            if (A.alloc(A.self, std::max<size_t>(tot.in, 1) * 8, &p) != RV_OK) return RV_E_NOMEM;
            S.ps.push_back(p), in_offs = (uint64_t*)p;
        }
        uint32_t* as_rec = S.get<uint32_t>(tot.as);
        uint64_t* as_op = S.get<uint64_t>(tot.as);
        uint32_t* pos = S.get<uint32_t>((size_t)n_levels + 1);
        CDNEED(as_rec && as_op && pos);
        if (n_wb64) k_z_wb_gates<<<blocks(W64, TB), TB, 0, st>>>(vbuf[wsort], seg_lo, seg_hi, wbx, W64, ops64, zc, s64, gates64 + n64);
        int lsort = 0;
        CDCHK(radix_sort(S, st, lk, lv, n64, bit_len(levels64), &lsort));
        k_cd_bounds<<<blocks(n64 + 1, TB), TB, 0, st>>>(lk[lsort], n64, n_levels, pos);
        k_z_gates<<<gb64, TB, 0, st>>>(lv[lsort], n64, ops64, prod, zc, orig64, s64, bx64, b2a_rows, gates64, rec_offs, in_offs, as_rec, as_op);
        CDCHK(hipGetLastError());
        cc.gates64.resize(n_g64);
        cc.rec_offs64.resize(n_rec64);
        cc.in_offs64.resize(tot.in);
        cc.assert_rec64.resize(tot.as);
        cc.assert_op64.resize(tot.as);
        auto d2h = [&](void* dst, const void* src, size_t bytes) { return bytes ? hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, st) : hipSuccess; };
        CDCHK(d2h(cc.gates64.data(), gates64, n_g64 * sizeof(Gate64)));
        CDCHK(d2h(cc.rec_offs64.data(), rec_offs, n_rec64 * 8));
        CDCHK(d2h(cc.in_offs64.data(), in_offs, (size_t)tot.in * 8));
        CDCHK(d2h(cc.assert_rec64.data(), as_rec, (size_t)tot.as * 4));
        CDCHK(d2h(cc.assert_op64.data(), as_op, (size_t)tot.as * 8));
        CDCHK(d2h(cc.level_start64.data(), pos, ((size_t)n_levels + 1) * 4));
        mark(3);
        CDCHK(hipStreamSynchronize(st));
        cc.level_start64[n_levels] = (uint32_t)n_g64;  // (the write-backs: the last level's, behind every op's gate)
        const uint64_t randoms = (uint64_t)tot.m - tot.in - 2ull * tot.mul - n_b2a;  // (a B2A's Z64 mask is not a Random op)
        cc.n_ssa64 = (uint64_t)s64.ssa_base + n64 - tot.as;
        cc.n_masks64 = n_masks64;
        cc.on_words64 = s64.on0 + tot.in + 8 * n_rec64;
        cc.pre_words64 = s64.pre0 + tot.mul + n_b2a;
        cc.n_in64 = tot.in;
        cc.n_rec64 = n_rec64;
        cc.n_corr64 = (uint64_t)tot.mul + n_b2a;
        cc.n_user_random += randoms;
        cc.info.z64_inputs = tot.in;
        cc.info.z64_muls = tot.mul;
        cc.info.z64_asserts = tot.as;
        cc.info.z64_linear = (uint64_t)n64 - tot.in - tot.mul - tot.as - n_b2a + n_wb64;
        cc.info.z64_masks = n_masks64;
        cc.info.b2a = n_b2a;
        if (laps) {
            float a = 0, b = 0, c = 0;
            (void)hipEventElapsedTime(&a, ev[0], ev[1]);
            (void)hipEventElapsedTime(&b, ev[2], ev[3]);
            (void)hipEventElapsedTime(&c, ev[4], ev[5]);
            laps->z64 = a + b + c;
            laps->levels = std::max(0.0f, laps->levels - c);  // (the Z64 levels ran inside the GF(2) compile's third step)
        }
        if (keep) {
            keep->d_gates64 = gates64;
            keep->d_rec_offs64 = rec_offs;
            keep->d_in_offs64 = in_offs;
            S.keep(gates64);
            S.keep(rec_offs);
            S.keep(in_offs);
        }
    }
    keep_guard.ok = true;
    return RV_OK;
}
}  // namespace

int compile_ops_device(hipStream_t st, const DevAlloc& A, const rv_op* d_ops, size_t n_ops, size_t z64_wires, size_t gf2_wires, bool keep_wires,
                       int force_lazy_k, Compiled& out, DevCompileKeep* keep, DevCompileLaps* laps, const ChunkStart* chunk, bool admit_z64,
                       bool admit_b2a) {
    if (keep) *keep = DevCompileKeep();
    if (admit_z64) return compile_mixed_device(st, A, d_ops, n_ops, z64_wires, gf2_wires, keep_wires, force_lazy_k, out, keep, laps, chunk, admit_b2a);
    return compile_gf2_device(st, A, d_ops, n_ops, z64_wires, gf2_wires, keep_wires, force_lazy_k, out, keep, laps, chunk, nullptr);
}
#undef CDCHK
#undef CDNEED

}  // namespace rv
