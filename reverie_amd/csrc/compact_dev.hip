// see compact_dev.h
//
// The sequential rule (compact.cpp) in parallel form, from the device compiler's building blocks (compile_dev_prims.inc: the scans, the
// radix sort, Scratch).  One thread per op in every kernel; no kernel waits for another workgroup.  The steps:
//   1. classify   the count in force at every op (an exclusive max-scan of the SizeHint fields), compile_ops' checks (the lowest bad
//                 op's index and code in one 64-bit word: atomicMin), the counts of values; with B2A ops, the pinned flags and
//                 their exclusive sum (the ranks; the total is P)
// then per domain (skipped when the list has no op of it):
//   2. writers    the defining ops sorted by destination index (stable: by op index within an index); an operand's value is the
//                 last entry of its index before the reading op (a binary search of the sorted pairs), none (the zero wire) or pinned
//   3. readers    atomicMax of reader index + 1 per value (0: dead)
//   4. counts     a_i (the op takes a slot) and f_i (slots it releases: operand a, operand b, its own dead value); with A the
//                 inclusive sum of a and F the exclusive sum of f, the fresh slots handed out through op i are
//                 N_i = max(0, max_{j <= i} (A_j - F_j)); op i is fresh iff a_i and N_i > N_{i-1}, and otherwise takes element
//                 A_i - N_i - 1 of the released sequence (written at F_i + k by the releasing ops): its parent
//   5. slots      parents followed to a fresh root by pointer doubling; the change flag is read once per four rounds
//   6. rewrite    dst, a, b and the SizeHints, each op by its own thread (so the output may be the input)
// The host reads device words three times outside the doubling loop: after step 1 (error word, counts in force: they size the sort),
// before step 6 (the consistency flag) and at the end (the info).
#include "compact_dev.h"

#include <algorithm>
#include <vector>

namespace rv {
namespace {
#include "compile_dev_prims.inc"
static_assert(TILE == COMPACT_TILE, "compact_dev.h names the scans' tile");

constexpr uint32_t NONE = 0xFFFFFFFFu;  // an operand on the zero wire
constexpr uint32_t PIN = 0xFFFFFFFEu;   // an operand on a pinned index
constexpr int G = 0, Z = 1;
// the words of one call in device memory
enum { S_ERR_LO, S_ERR_HI, S_HINT_Z, S_HINT_G, S_VALUES_G, S_VALUES_Z, S_B2A, S_OPS_G, S_OPS_Z, S_P, S_ZERO_G, S_ZERO_Z, S_FRESH_G, S_FRESH_Z, S_BAD,
       S_WORDS };
constexpr int MAX_ROUNDS = 36, ROUNDS_PER_LOOK = 4;

__device__ inline int op_reads(uint32_t opcode) {
    return (opcode == RV_OP_ADD || opcode == RV_OP_SUB || opcode == RV_OP_MUL)                                          ? 2
           : (opcode == RV_OP_ADDCONST || opcode == RV_OP_SUBCONST || opcode == RV_OP_MULCONST || opcode == RV_OP_ASSERTZERO) ? 1
                                                                                                                             : 0;
}
// the domain whose pool the op's value belongs to (-1: the op defines none), pinned destinations included
__device__ inline int value_dom(const rv_op& op) {
    if (op.domain == RV_DOM_B2A) return Z;
    if (op.domain > RV_DOM_Z64 || op.opcode == RV_OP_ASSERTZERO) return -1;
    return op.domain == RV_DOM_GF2 ? G : Z;
}
__device__ inline bool pinned(const uint32_t* pins, uint32_t w) { return pins && pins[w]; }
// the op takes a pool slot of domain d
__device__ inline bool takes_slot(const rv_op& op, int d, const uint32_t* pins) {
    return value_dom(op) == d && !(op.domain == RV_DOM_GF2 && pinned(pins, op.dst));
}

// ---- step 1 (the hints: compile_dev_prims.inc's k_pr_hints) ----
__global__ __launch_bounds__(TB) void k_cw_classify(const rv_op* ops, size_t n, uint64_t decl_z, uint64_t decl_g, const uint32_t* cz, const uint32_t* cg,
                                                    uint32_t* state) {
    __shared__ uint32_t cnt[5];  // values G, values Z, B2A, ops G, ops Z
    if (threadIdx.x < 5) cnt[threadIdx.x] = 0;
    __syncthreads();
    const size_t i = (size_t)blockIdx.x * TB + threadIdx.x;
    if (i < n) {
        const rv_op op = ops[i];
        const uint64_t nz = decl_z > cz[i] ? decl_z : cz[i], ng = decl_g > cg[i] ? decl_g : cg[i];
        int rc = RV_OK;
        if (op.reserved != 0) {
            rc = RV_E_BAD_OP;
        } else if (op.domain == RV_DOM_GF2 || op.domain == RV_DOM_Z64) {
            const uint64_t nw = op.domain == RV_DOM_GF2 ? ng : nz;
            const int r = op_reads(op.opcode);
            if (op.opcode > RV_OP_CONST) rc = RV_E_BAD_OP;
            else if ((op.opcode != RV_OP_ASSERTZERO && op.dst >= nw) || (r >= 1 && op.a >= nw) || (r >= 2 && op.b >= nw)) rc = RV_E_WIRE_OOB;
        } else if (op.domain == RV_DOM_B2A) {
            if (op.dst >= nz || (uint64_t)op.a + 64 > ng) rc = RV_E_WIRE_OOB;
        } else if (op.domain != RV_DOM_SIZEHINT) {
            rc = RV_E_BAD_OP;
        }
        if (rc != RV_OK) {
            atomicMin((unsigned long long*)state, ((unsigned long long)i << 8) | (unsigned long long)rc);
        } else {
            const int d = value_dom(op);
            if (d >= 0) atomicAdd(&cnt[d], 1u);
            if (op.domain == RV_DOM_B2A) atomicAdd(&cnt[2], 1u);
            if (op.domain == RV_DOM_GF2) atomicAdd(&cnt[3], 1u);
            if (op.domain == RV_DOM_Z64 || op.domain == RV_DOM_B2A) atomicAdd(&cnt[4], 1u);
        }
    }
    __syncthreads();
    if (threadIdx.x < 5 && cnt[threadIdx.x]) atomicAdd(&state[S_VALUES_G + threadIdx.x], cnt[threadIdx.x]);
}
// (after the checks passed: every range lies below the GF(2) count in force, the length of `pins`)
__global__ __launch_bounds__(TB) void k_cw_pins(const rv_op* ops, size_t n, uint32_t* pins, uint32_t W) {
    const size_t i = (size_t)blockIdx.x * TB + threadIdx.x;
    if (i >= n || ops[i].domain != RV_DOM_B2A) return;
    const uint32_t a = ops[i].a;
    for (uint32_t k = 0; k < 64; k++)
        if (a + k < W) pins[a + k] = 1u;
}
__global__ __launch_bounds__(TB) void k_cw_iota(uint32_t* par, size_t n) {
    const size_t i = (size_t)blockIdx.x * TB + threadIdx.x;
    if (i < n) par[i] = (uint32_t)i;
}

// ---- step 2 ----
__global__ __launch_bounds__(TB) void k_cw_keys(const rv_op* ops, size_t n, int d, uint32_t W, const uint32_t* pins, uint32_t* key, uint32_t* idx) {
    const size_t i = (size_t)blockIdx.x * TB + threadIdx.x;
    if (i >= n) return;
    const rv_op op = ops[i];
    key[i] = takes_slot(op, d, pins) ? op.dst : W;
    idx[i] = (uint32_t)i;
}
// the value on index w that op i reads: the last pair (w, j) with j < i of the sorted (index, op) pairs
__device__ inline uint32_t value_read(const uint32_t* sk, const uint32_t* sv, uint32_t n, uint32_t w, uint32_t i) {
    uint32_t lo = 0, hi = n;
    while (lo < hi) {  // (at most 32 steps)
        const uint32_t mid = lo + (hi - lo) / 2;
        const uint32_t k = sk[mid];
        if (k < w || (k == w && sv[mid] < i)) lo = mid + 1;
        else hi = mid;
    }
    return (lo > 0 && sk[lo - 1] == w) ? sv[lo - 1] : NONE;
}
// steps 2 and 3 for the ops of domain d
__global__ __launch_bounds__(TB) void k_cw_resolve(const rv_op* ops, size_t n, int d, const uint32_t* sk, const uint32_t* sv, const uint32_t* pins,
                                                   uint32_t* va, uint32_t* vb, uint32_t* last, uint32_t* state) {
    const size_t i = (size_t)blockIdx.x * TB + threadIdx.x;
    if (i >= n) return;
    const rv_op op = ops[i];
    if (op.domain != (d == G ? RV_DOM_GF2 : RV_DOM_Z64)) return;
    const int r = op_reads(op.opcode);
    for (int k = 0; k < r; k++) {
        const uint32_t w = k ? op.b : op.a;
        uint32_t v;
        if (d == G && pinned(pins, w)) {
            v = PIN;
        } else {
            v = value_read(sk, sv, (uint32_t)n, w, (uint32_t)i);
            if (v == NONE) state[d == G ? S_ZERO_G : S_ZERO_Z] = 1u;  // (every writer stores the same word)
            else atomicMax(&last[v], (uint32_t)i + 1u);
        }
        (k ? vb : va)[i] = v;
    }
}

// ---- step 4 ----
// the values op i releases, in the rule's order, into out[0..3); returns how many
__device__ inline int releases(const rv_op& op, uint32_t i, int d, bool takes, const uint32_t* va, const uint32_t* vb, const uint32_t* last, uint32_t out[3]) {
    int f = 0;
    if (op.domain == (d == G ? RV_DOM_GF2 : RV_DOM_Z64)) {
        const int r = op_reads(op.opcode);
        const uint32_t a = r >= 1 ? va[i] : NONE, b = r >= 2 ? vb[i] : NONE;
        if (a < PIN && last[a] == i + 1u) out[f++] = a;
        if (b < PIN && b != a && last[b] == i + 1u) out[f++] = b;
    }
    if (takes && last[i] == 0u) out[f++] = i;
    return f;
}
__global__ __launch_bounds__(TB) void k_cw_counts(const rv_op* ops, size_t n, int d, const uint32_t* pins, const uint32_t* va, const uint32_t* vb,
                                                  const uint32_t* last, uint32_t* al, uint32_t* fr) {
    const size_t i = (size_t)blockIdx.x * TB + threadIdx.x;
    if (i >= n) return;
    const rv_op op = ops[i];
    const bool takes = takes_slot(op, d, pins);
    uint32_t rel[3];
    al[i] = takes ? 1u : 0u;
    fr[i] = (uint32_t)releases(op, (uint32_t)i, d, takes, va, vb, last, rel);
}
__global__ __launch_bounds__(TB) void k_cw_demand(const uint32_t* al, const uint32_t* a_ex, const uint32_t* f_ex, size_t n, uint32_t* dp) {
    const size_t i = (size_t)blockIdx.x * TB + threadIdx.x;
    if (i >= n) return;
    const uint32_t a = a_ex[i] + al[i], f = f_ex[i];
    dp[i] = a > f ? a - f : 0u;
}
__global__ __launch_bounds__(TB) void k_cw_released(const rv_op* ops, size_t n, int d, const uint32_t* al, const uint32_t* va, const uint32_t* vb,
                                                    const uint32_t* last, const uint32_t* f_ex, uint32_t* relseq) {
    const size_t i = (size_t)blockIdx.x * TB + threadIdx.x;
    if (i >= n) return;
    const rv_op op = ops[i];
    uint32_t rel[3];
    const int f = releases(op, (uint32_t)i, d, al[i] != 0, va, vb, last, rel);
    for (int k = 0; k < f; k++)
        if ((size_t)f_ex[i] + k < n) relseq[f_ex[i] + k] = rel[k];
}
// a fresh op is its own root and has its slot; any other takes the op whose released slot it reuses as its parent
__global__ __launch_bounds__(TB) void k_cw_parents(size_t n, int d, const uint32_t* al, const uint32_t* a_ex, const uint32_t* f_ex, const uint32_t* dp,
                                                   const uint32_t* n_ex, const uint32_t* relseq, uint32_t* state, uint32_t* par, uint32_t* slot) {
    const size_t i = (size_t)blockIdx.x * TB + threadIdx.x;
    if (i >= n || !al[i]) return;
    const uint32_t base = d == G ? state[S_P] + state[S_ZERO_G] : state[S_ZERO_Z];
    const uint32_t before = n_ex[i], through = max(before, dp[i]);
    if (through > before) {
        slot[i] = base + through - 1u;
        return;
    }
    const uint32_t at = a_ex[i] - through;  // A_i - N_i - 1 (A_i = a_ex[i] + 1)
    if (at >= f_ex[i]) {  // (cannot happen: a reused slot was released by an earlier op)
        state[S_BAD] = 1u;
        return;
    }
    par[i] = relseq[at];
}

// ---- step 5 ----
__global__ __launch_bounds__(TB) void k_cw_jump(uint32_t* par, size_t n, uint32_t* changed) {
    const size_t i = (size_t)blockIdx.x * TB + threadIdx.x;
    if (i >= n) return;
    const uint32_t p = par[i];
    if (p == (uint32_t)i) return;
    const uint32_t pp = par[p];  // (a parent written in this round is an ancestor too)
    if (pp != p) {
        par[i] = pp;
        *changed = 1u;
    }
}
__global__ __launch_bounds__(TB) void k_cw_slots(size_t n, const uint32_t* al, const uint32_t* par, uint32_t* slot) {
    const size_t i = (size_t)blockIdx.x * TB + threadIdx.x;
    if (i >= n || !al[i]) return;
    const uint32_t p = par[i];
    if (p != (uint32_t)i) slot[i] = slot[p];  // (p is a root: its slot is written by no thread here)
}

// ---- step 6 ----
__global__ __launch_bounds__(TB) void k_cw_rewrite(const rv_op* ops, size_t n, const uint32_t* pins, const uint32_t* rank, const uint32_t* va,
                                                   const uint32_t* vb, const uint32_t* slot, const uint32_t* state, rv_op* out) {
    const size_t i = (size_t)blockIdx.x * TB + threadIdx.x;
    if (i >= n) return;
    rv_op op = ops[i];
    const uint32_t P = state[S_P];
    if (op.domain == RV_DOM_SIZEHINT) {
        op.a = state[S_ZERO_Z] + state[S_FRESH_Z];
        op.b = P + state[S_ZERO_G] + state[S_FRESH_G];
    } else if (op.domain == RV_DOM_B2A) {
        op.a = rank[op.a];
        op.dst = slot[i];
    } else {
        const int d = op.domain == RV_DOM_GF2 ? G : Z;
        const int r = op_reads(op.opcode);
        if (r >= 1) {
            const uint32_t v = va[i];
            op.a = v == PIN ? rank[op.a] : v == NONE ? (d == G ? P : 0u) : slot[v];
        }
        if (r >= 2) {
            const uint32_t v = vb[i];
            op.b = v == PIN ? rank[op.b] : v == NONE ? (d == G ? P : 0u) : slot[v];
        }
        if (op.opcode != RV_OP_ASSERTZERO) op.dst = (d == G && pinned(pins, op.dst)) ? rank[op.dst] : slot[i];
    }
    out[i] = op;
}

// the arrays one call keeps across its steps
struct Work {
    uint32_t *state, *pins, *rank, *va, *vb, *last, *par, *slot;
    uint32_t *kbuf[2], *vbuf[2], *al, *fr, *a_ex, *f_ex, *dp, *n_ex, *relseq, *changed;
};

// steps 2 - 5 of domain d
int domain_pass(Scratch& S, hipStream_t st, const rv_op* ops, size_t n, int d, uint32_t W, Work& w) {
    const uint32_t gb = blocks(n, TB);
    k_cw_keys<<<gb, TB, 0, st>>>(ops, n, d, W, w.pins, w.kbuf[0], w.vbuf[0]);
    int which = 0;
    CDCHK(radix_sort(S, st, w.kbuf, w.vbuf, n, bit_len(W), &which));
    k_cw_resolve<<<gb, TB, 0, st>>>(ops, n, d, w.kbuf[which], w.vbuf[which], w.pins, w.va, w.vb, w.last, w.state);
    k_cw_counts<<<gb, TB, 0, st>>>(ops, n, d, w.pins, w.va, w.vb, w.last, w.al, w.fr);
    CDCHK(hipGetLastError());
    CDCHK((scan_excl<uint32_t, SumU32>(S, st, w.al, w.a_ex, n, nullptr)));
    CDCHK((scan_excl<uint32_t, SumU32>(S, st, w.fr, w.f_ex, n, nullptr)));
    k_cw_demand<<<gb, TB, 0, st>>>(w.al, w.a_ex, w.f_ex, n, w.dp);
    CDCHK((scan_excl<uint32_t, MaxU32>(S, st, w.dp, w.n_ex, n, &w.state[d == G ? S_FRESH_G : S_FRESH_Z])));
    k_cw_released<<<gb, TB, 0, st>>>(ops, n, d, w.al, w.va, w.vb, w.last, w.f_ex, w.relseq);
    k_cw_parents<<<gb, TB, 0, st>>>(n, d, w.al, w.a_ex, w.f_ex, w.dp, w.n_ex, w.relseq, w.state, w.par, w.slot);
    CDCHK(hipGetLastError());
    CDCHK(hipMemsetAsync(w.changed, 0, MAX_ROUNDS * 4, st));
    for (int r = 0; r < MAX_ROUNDS; r++) {
        k_cw_jump<<<gb, TB, 0, st>>>(w.par, n, w.changed + r);
        if (r % ROUNDS_PER_LOOK == ROUNDS_PER_LOOK - 1) {
            uint32_t c = 0;
            CDCHK(hipMemcpyAsync(&c, w.changed + r, 4, hipMemcpyDeviceToHost, st));
            CDCHK(hipStreamSynchronize(st));
            if (!c) break;
        }
    }
    k_cw_slots<<<gb, TB, 0, st>>>(n, w.al, w.par, w.slot);
    CDCHK(hipGetLastError());
    return RV_OK;
}

int compact_impl(hipStream_t st, const DevAlloc& A, const rv_op* ops, size_t n, uint64_t z64_wires, uint64_t gf2_wires, rv_op* out, rv_compact_info* info) {
    Scratch S(A, st);
    const uint32_t gb = blocks(n, TB);
    Work w{};
    w.state = S.get<uint32_t>(S_WORDS);
    for (int k = 0; k < 2; k++) w.kbuf[k] = S.get<uint32_t>(n), w.vbuf[k] = S.get<uint32_t>(n);
    CDNEED(w.state && w.kbuf[0] && w.kbuf[1] && w.vbuf[0] && w.vbuf[1]);
    std::vector<uint32_t> h(S_WORDS);

    // step 1 (the hints and their scans borrow the sort's buffers)
    CDCHK(hipMemsetAsync(w.state, 0, S_WORDS * 4, st));
    CDCHK(hipMemsetAsync(w.state, 0xFF, 8, st));
    k_pr_hints<<<gb, TB, 0, st>>>(ops, n, w.kbuf[0], w.kbuf[1]);
    CDCHK((scan_excl<uint32_t, MaxU32>(S, st, w.kbuf[0], w.vbuf[0], n, &w.state[S_HINT_Z])));
    CDCHK((scan_excl<uint32_t, MaxU32>(S, st, w.kbuf[1], w.vbuf[1], n, &w.state[S_HINT_G])));
    k_cw_classify<<<gb, TB, 0, st>>>(ops, n, z64_wires, gf2_wires, w.vbuf[0], w.vbuf[1], w.state);
    CDCHK(hipGetLastError());
    CDCHK(fetch(st, h, w.state));
    CDCHK(hipStreamSynchronize(st));
    if (h[S_ERR_HI] != 0xFFFFFFFFu || h[S_ERR_LO] != 0xFFFFFFFFu) return (int)(h[S_ERR_LO] & 0xFFu);
    const uint64_t Wz = std::max<uint64_t>(z64_wires, h[S_HINT_Z]), Wg = std::max<uint64_t>(gf2_wires, h[S_HINT_G]);
    if (Wz >= (1ull << 31) || Wg >= (1ull << 31)) return RV_E_UNSUPPORTED;

    if (h[S_B2A]) {
        w.pins = S.get<uint32_t>(Wg);
        w.rank = S.get<uint32_t>(Wg);
        CDNEED(w.pins && w.rank);
        CDCHK(hipMemsetAsync(w.pins, 0, std::max<size_t>(Wg, 1) * 4, st));
        k_cw_pins<<<gb, TB, 0, st>>>(ops, n, w.pins, (uint32_t)Wg);
        CDCHK((scan_excl<uint32_t, SumU32>(S, st, w.pins, w.rank, Wg, &w.state[S_P])));
    }
    w.va = S.get<uint32_t>(n), w.vb = S.get<uint32_t>(n), w.last = S.get<uint32_t>(n), w.par = S.get<uint32_t>(n), w.slot = S.get<uint32_t>(n);
    w.al = S.get<uint32_t>(n), w.fr = S.get<uint32_t>(n), w.a_ex = S.get<uint32_t>(n), w.f_ex = S.get<uint32_t>(n), w.dp = S.get<uint32_t>(n);
    w.n_ex = S.get<uint32_t>(n), w.relseq = S.get<uint32_t>(n), w.changed = S.get<uint32_t>(MAX_ROUNDS);
    CDNEED(w.va && w.vb && w.last && w.par && w.slot && w.al && w.fr && w.a_ex && w.f_ex && w.dp && w.n_ex && w.relseq && w.changed);
    CDCHK(hipMemsetAsync(w.last, 0, n * 4, st));
    k_cw_iota<<<gb, TB, 0, st>>>(w.par, n);
    CDCHK(hipGetLastError());
    if (h[S_OPS_G])
        if (const int rc = domain_pass(S, st, ops, n, G, (uint32_t)Wg, w)) return rc;
    if (h[S_OPS_Z])
        if (const int rc = domain_pass(S, st, ops, n, Z, (uint32_t)Wz, w)) return rc;

    CDCHK(fetch(st, h, w.state));
    CDCHK(hipStreamSynchronize(st));
    if (h[S_BAD]) return RV_E_DEVICE;
    k_cw_rewrite<<<gb, TB, 0, st>>>(ops, n, w.pins, w.rank, w.va, w.vb, w.slot, w.state, out);
    CDCHK(hipGetLastError());
    CDCHK(hipStreamSynchronize(st));
    if (info) {
        *info = rv_compact_info{};
        info->z64_wires = (uint64_t)h[S_ZERO_Z] + h[S_FRESH_Z], info->gf2_wires = (uint64_t)h[S_P] + h[S_ZERO_G] + h[S_FRESH_G];
        info->gf2_pinned = h[S_P], info->gf2_zero_wire = h[S_ZERO_G], info->z64_zero_wire = h[S_ZERO_Z];
        info->gf2_values = h[S_VALUES_G], info->z64_values = h[S_VALUES_Z];
    }
    return RV_OK;
}
#undef CDCHK
#undef CDNEED
}  // namespace

int compact_ops_device(hipStream_t st, const DevAlloc& A, const rv_op* d_ops, size_t n_ops, uint64_t z64_wires, uint64_t gf2_wires, rv_op* d_out,
                       rv_compact_info* info) {
    if (n_ops >= (1ull << 31)) return RV_E_UNSUPPORTED;
    if (n_ops == 0) {
        if (info) *info = rv_compact_info{};
        return RV_OK;
    }
    return compact_impl(st, A, d_ops, n_ops, z64_wires, gf2_wires, d_out, info);
}

}  // namespace rv
