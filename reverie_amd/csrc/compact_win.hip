// see compact_win.h
//
// compact_dev.hip's rule for a list that arrives in feeds.  Two passes; one thread per op of the feed in every kernel,
// no kernel waits for another workgroup, the building blocks are compile_dev_prims.inc's.
//
// Scan pass.  Carried per domain and old wire index w: def[w], the ordinal of the op that defined the value now on w (NONE: none),
// and rd[w], that value's last reader so far as ((ordinal << 1 | slot is a) + 1) (0: none) -- a maximum, so the latest reader wins
// and, where a and b of one op name the value, the slot is a.  One mark byte per op of the whole list: this op releases operand a /
// operand b / its own dead value, takes a pool slot, its pool is Z64's.  A feed sorts its defining ops by destination index (stable);
// an operand reads the last in-feed definition before its op, else the carried value (rd[w] by atomicMax), else the zero wire.  A
// value is final when the feed defines its index again (the carried one, and every in-feed one but the group's last, which becomes
// the carried one) or when the list ends: one atomicOr into the mark word of its last reader, or of its definer when nothing read it
// -- an op of any earlier feed, which is why the marks are resident.  At the end the marks alone give the fresh-slot counts
// (N = max over ops of A_i - F_i, per block of 256 ops and combined on the host), hence the new wire counts, before the rewrite pass
// needs them.  With a B2A op the pinned indices are known only at the end of the list and decide which ops take slots: the pass is
// run twice, the first time for the validation and the pin table.
//
// Rewrite pass.  Carried per domain: slotof[w], the new slot of the value now on w (in def[]'s place), the free slots as a ring of
// resolved slot numbers, the fresh counter.  A feed is compact_dev.hip's steps 4 - 6 with a carry-in: the released sequence is the
// carried ring (length L) followed by the feed's own releases; with A the inclusive count of slot-taking ops and F the exclusive
// count of releases inside the feed, N_i = max(0, max_{j <= i}(A_j - L - F_j)) slots are fresh through op i.  A taking op that is
// not fresh takes element A_i - N_i - 1 of the sequence: below L a ring entry (a root), otherwise a released value that is either
// carried (its slot is known: a root) or an op of the feed (a parent, followed by pointer doubling).  What the feed did not consume
// stays in the ring, its releases appended as slot numbers.  The marks stand in for last[].
#include "compact_win.h"

#include <algorithm>
#include <vector>

#include "win_stage.h"

namespace rv {
namespace {
#include "compile_dev_prims.inc"

constexpr uint32_t NONE = 0xFFFFFFFFu;  // an operand on the zero wire; an index without a value
constexpr uint32_t PIN = 0xFFFFFFFEu;   // an operand on a pinned index
constexpr uint32_t TAG = 0x80000000u;   // TAG | slot: a value from before the feed, by its slot (slots stay below 2^31 - 2)
constexpr uint32_t MAX_SLOTS = 0x7FFFFFF0u;
constexpr int G = 0, Z = 1;
constexpr uint32_t M_REL_A = 1, M_REL_B = 2, M_DEAD = 4, M_TAKES = 8, M_DOMZ = 16;
// the words of one compactor in device memory; [S_FEED_FIRST, S_WORDS) are one feed's and cleared when it begins
enum { S_P, S_ZERO_G, S_ZERO_Z, S_BAD, S_FEED_FIRST, S_ERR_LO = S_FEED_FIRST, S_ERR_HI, S_HINT_Z, S_HINT_G, S_VALUES_G, S_VALUES_Z, S_B2A, S_OPS_G, S_OPS_Z,
       S_ATOT_G, S_ATOT_Z, S_FTOT_G, S_FTOT_Z, S_NLOC_G, S_NLOC_Z, S_WORDS };
static_assert(S_ERR_LO % 2 == 0, "the error word is one aligned 64-bit word");
static_assert(S_WORDS * 4 <= WIN_CUT_AT, "the state words are the start of the stage's block");
constexpr int MAX_ROUNDS = 36, ROUNDS_PER_LOOK = 4;
constexpr int RB = 256;  // ops per block of the marks' reduction

__device__ inline int op_reads(uint32_t opcode) {
    return (opcode == RV_OP_ADD || opcode == RV_OP_SUB || opcode == RV_OP_MUL)                                          ? 2
           : (opcode == RV_OP_ADDCONST || opcode == RV_OP_SUBCONST || opcode == RV_OP_MULCONST || opcode == RV_OP_ASSERTZERO) ? 1
                                                                                                                             : 0;
}
__device__ inline int value_dom(const rv_op& op) {
    if (op.domain == RV_DOM_B2A) return Z;
    if (op.domain > RV_DOM_Z64 || op.opcode == RV_OP_ASSERTZERO) return -1;
    return op.domain == RV_DOM_GF2 ? G : Z;
}
// (w below the table's length W: a rescan or a rewrite pass is not validated again, so every index is looked at before it is used)
__device__ inline bool pinned(const uint32_t* pins, uint32_t w, uint32_t Wg) { return pins && w < Wg && pins[w]; }
__device__ inline bool takes_slot(const rv_op& op, int d, const uint32_t* pins, uint32_t Wg) {
    return value_dom(op) == d && !(op.domain == RV_DOM_GF2 && pinned(pins, op.dst, Wg));
}
__device__ inline void mark_or(uint32_t* marks, uint64_t total, uint64_t ord, uint32_t bits) {
    if (ord < total) atomicOr(&marks[ord >> 2], bits << (8u * (uint32_t)(ord & 3u)));
}
__device__ inline uint32_t mark_of(const uint32_t* marks, uint64_t ord) { return (marks[ord >> 2] >> (8u * (uint32_t)(ord & 3u))) & 0xFFu; }
// the value (definer ordinal dv, last reader key r) is final
__device__ inline void finalise(uint32_t* marks, uint64_t total, uint32_t dv, uint32_t r) {
    if (r == 0u) mark_or(marks, total, dv, M_DEAD);
    else mark_or(marks, total, (r - 1u) >> 1, ((r - 1u) & 1u) ? M_REL_A : M_REL_B);
}

// ---- validation (first scan pass): compact_dev.hip's step 1 with the counts in force carried in (the hints: k_pr_hints) ----
__global__ __launch_bounds__(TB) void k_w_classify(const rv_op* ops, size_t n, uint64_t in_z, uint64_t in_g, const uint32_t* cz, const uint32_t* cg,
                                                   uint32_t* state) {
    __shared__ uint32_t cnt[5];  // values G, values Z, B2A, ops G, ops Z
    if (threadIdx.x < 5) cnt[threadIdx.x] = 0;
    __syncthreads();
    const size_t i = (size_t)blockIdx.x * TB + threadIdx.x;
    if (i < n) {
        const rv_op op = ops[i];
        const uint64_t nz = in_z > cz[i] ? in_z : cz[i], ng = in_g > cg[i] ? in_g : cg[i];
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
            atomicMin((unsigned long long*)&state[S_ERR_LO], ((unsigned long long)i << 8) | (unsigned long long)rc);
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
__global__ __launch_bounds__(TB) void k_w_pins(const rv_op* ops, size_t n, uint32_t* pins, uint32_t Wg) {
    const size_t i = (size_t)blockIdx.x * TB + threadIdx.x;
    if (i >= n || ops[i].domain != RV_DOM_B2A) return;
    const uint32_t a = ops[i].a;
    for (uint32_t k = 0; k < 64; k++)
        if ((uint64_t)a + k < Wg) pins[a + k] = 1u;
}
__global__ __launch_bounds__(TB) void k_w_iota(uint32_t* par, size_t n) {
    const size_t i = (size_t)blockIdx.x * TB + threadIdx.x;
    if (i < n) par[i] = (uint32_t)i;
}

// ---- both passes: the feed's defining ops by destination index ----
__global__ __launch_bounds__(TB) void k_w_keys(const rv_op* ops, size_t n, int d, uint32_t W, const uint32_t* pins, uint32_t Wg, uint32_t* key,
                                               uint32_t* idx) {
    const size_t i = (size_t)blockIdx.x * TB + threadIdx.x;
    if (i >= n) return;
    const rv_op op = ops[i];
    key[i] = (takes_slot(op, d, pins, Wg) && op.dst < W) ? op.dst : W;
    idx[i] = (uint32_t)i;
}
__device__ inline uint32_t value_read(const uint32_t* sk, const uint32_t* sv, uint32_t n, uint32_t w, uint32_t i) {
    uint32_t lo = 0, hi = n;
    while (lo < hi) {
        const uint32_t mid = lo + (hi - lo) / 2;
        const uint32_t k = sk[mid];
        if (k < w || (k == w && sv[mid] < i)) lo = mid + 1;
        else hi = mid;
    }
    return (lo > 0 && sk[lo - 1] == w) ? sv[lo - 1] : NONE;
}

// ---- scan pass ----
// the op's own bits (plain byte stores: no other kernel of the feed has touched these bytes yet, and the next ones come after this one)
__global__ __launch_bounds__(TB) void k_w_own(const rv_op* ops, size_t n, uint64_t pos, const uint32_t* pins, uint32_t Wg, uint8_t* marks) {
    const size_t i = (size_t)blockIdx.x * TB + threadIdx.x;
    if (i >= n) return;
    const rv_op op = ops[i];
    uint32_t m = (op.domain == RV_DOM_Z64 || op.domain == RV_DOM_B2A) ? M_DOMZ : 0u;
    if (takes_slot(op, G, pins, Wg) || takes_slot(op, Z, pins, Wg)) m |= M_TAKES;
    marks[pos + i] = (uint8_t)m;
}
__global__ __launch_bounds__(TB) void k_w_scan_reads(const rv_op* ops, size_t n, uint64_t pos, int d, uint32_t W, const uint32_t* sk, const uint32_t* sv,
                                                     const uint32_t* pins, uint32_t Wg, const uint32_t* def, uint32_t* rd, uint32_t* last, uint32_t* state) {
    const size_t i = (size_t)blockIdx.x * TB + threadIdx.x;
    if (i >= n) return;
    const rv_op op = ops[i];
    if (op.domain != (d == G ? RV_DOM_GF2 : RV_DOM_Z64)) return;
    const int r = op_reads(op.opcode);
    for (int k = 0; k < r; k++) {
        const uint32_t w = k ? op.b : op.a;
        if (d == G && pinned(pins, w, Wg)) continue;
        if (w >= W) {
            state[S_BAD] = 1u;
            continue;
        }
        const uint32_t key = ((((uint32_t)(pos + i)) << 1) | (k == 0 ? 1u : 0u)) + 1u;
        const uint32_t v = value_read(sk, sv, (uint32_t)n, w, (uint32_t)i);
        if (v != NONE) atomicMax(&last[v], key);
        else if (def[w] == NONE) state[d == G ? S_ZERO_G : S_ZERO_Z] = 1u;  // (every writer stores the same word)
        else atomicMax(&rd[w], key);
    }
}
// one thread per sorted pair; the last definition of an index in the feed finalises the carried value and takes its place
__global__ __launch_bounds__(TB) void k_w_scan_defs(size_t n, uint64_t pos, uint32_t W, const uint32_t* sk, const uint32_t* sv, const uint32_t* last,
                                                    uint32_t* def, uint32_t* rd, uint32_t* marks, uint64_t total) {
    const size_t j = (size_t)blockIdx.x * TB + threadIdx.x;
    if (j >= n) return;
    const uint32_t w = sk[j];
    if (w >= W) return;
    const uint32_t i = sv[j];
    const bool is_last = j + 1 == n || sk[j + 1] != w;
    if (!is_last) {
        finalise(marks, total, (uint32_t)(pos + i), last[i]);
    } else {
        const uint32_t dv = def[w];
        if (dv != NONE) finalise(marks, total, dv, rd[w]);
        def[w] = (uint32_t)(pos + i);
        rd[w] = last[i];
    }
}
__global__ __launch_bounds__(TB) void k_w_scan_rest(uint32_t W, const uint32_t* def, const uint32_t* rd, uint32_t* marks, uint64_t total) {
    const size_t w = (size_t)blockIdx.x * TB + threadIdx.x;
    if (w >= W) return;
    if (def[w] != NONE) finalise(marks, total, def[w], rd[w]);
}
// per block of RB ops and per domain: slots taken, slots released, max over its ops of (taken through the op - released before it)
__global__ __launch_bounds__(RB) void k_w_marks_reduce(const uint32_t* marks, uint64_t total, int32_t* out) {
    static_assert(RB == TB, "block_excl scans TB values");
    __shared__ uint32_t sh[TB];
    __shared__ int32_t mx[2];
    if (threadIdx.x < 2) mx[threadIdx.x] = -0x7FFFFFFF;
    const uint64_t i = (uint64_t)blockIdx.x * RB + threadIdx.x;
    const uint32_t m = i < total ? mark_of(marks, i) : 0u;
    const int md = (m & M_DOMZ) ? Z : G;
    const uint32_t rel = (uint32_t)__popc(m & 7u);
    for (int d = 0; d < 2; d++) {
        const uint32_t a = (md == d && (m & M_TAKES)) ? 1u : 0u, f = md == d ? rel : 0u;
        uint32_t ta, tf;
        const uint32_t ea = block_excl<uint32_t, SumU32>(a, sh, &ta);
        const uint32_t ef = block_excl<uint32_t, SumU32>(f, sh, &tf);
        if (a) atomicMax(&mx[d], (int32_t)(ea + 1u) - (int32_t)ef);
        __syncthreads();
        if (threadIdx.x == 0) {
            int32_t* o = out + ((size_t)blockIdx.x * 2 + d) * 3;
            o[0] = (int32_t)ta, o[1] = (int32_t)tf, o[2] = mx[d];
        }
    }
}

// ---- rewrite pass ----
__global__ __launch_bounds__(TB) void k_w_rw_reads(const rv_op* ops, size_t n, int d, uint32_t W, const uint32_t* sk, const uint32_t* sv, const uint32_t* pins,
                                                   uint32_t Wg, const uint32_t* slotof, uint32_t* va, uint32_t* vb, uint32_t* state) {
    const size_t i = (size_t)blockIdx.x * TB + threadIdx.x;
    if (i >= n) return;
    const rv_op op = ops[i];
    if (op.domain != (d == G ? RV_DOM_GF2 : RV_DOM_Z64)) return;
    const int r = op_reads(op.opcode);
    for (int k = 0; k < r; k++) {
        const uint32_t w = k ? op.b : op.a;
        uint32_t v;
        if (d == G && pinned(pins, w, Wg)) {
            v = PIN;
        } else if (w >= W) {
            state[S_BAD] = 1u;
            v = NONE;
        } else {
            v = value_read(sk, sv, (uint32_t)n, w, (uint32_t)i);
            if (v == NONE && slotof[w] != NONE) v = TAG | slotof[w];
        }
        (k ? vb : va)[i] = v;
    }
}
__global__ __launch_bounds__(TB) void k_w_rw_counts(size_t n, uint64_t pos, int d, const uint32_t* marks, uint32_t* al, uint32_t* fr) {
    const size_t i = (size_t)blockIdx.x * TB + threadIdx.x;
    if (i >= n) return;
    const uint32_t m = mark_of(marks, pos + i);
    const bool mine = ((m & M_DOMZ) ? Z : G) == d;
    al[i] = (mine && (m & M_TAKES)) ? 1u : 0u;
    fr[i] = mine ? (uint32_t)__popc(m & 7u) : 0u;
}
__global__ __launch_bounds__(TB) void k_w_rw_demand(const uint32_t* al, const uint32_t* a_ex, const uint32_t* f_ex, size_t n, uint32_t L, uint32_t* dp) {
    const size_t i = (size_t)blockIdx.x * TB + threadIdx.x;
    if (i >= n) return;
    const uint64_t a = (uint64_t)a_ex[i] + al[i], f = (uint64_t)f_ex[i] + L;
    dp[i] = a > f ? (uint32_t)(a - f) : 0u;
}
// relseq: 3 n entries (an op releases at most three values; its own feed need not have defined any of them)
__global__ __launch_bounds__(TB) void k_w_rw_released(size_t n, uint64_t pos, int d, const uint32_t* marks, const uint32_t* va, const uint32_t* vb,
                                                      const uint32_t* f_ex, uint32_t* relseq, uint32_t* state) {
    const size_t i = (size_t)blockIdx.x * TB + threadIdx.x;
    if (i >= n) return;
    const uint32_t m = mark_of(marks, pos + i);
    if (((m & M_DOMZ) ? Z : G) != d || !(m & 7u)) return;
    size_t at = f_ex[i];
    const uint32_t rel[3] = {va[i], vb[i], (uint32_t)i};
    for (int k = 0; k < 3; k++) {
        if (!(m & (1u << k))) continue;
        const uint32_t v = rel[k];
        if (k < 2 && (v == NONE || v == PIN || (!(v & TAG) && v >= i))) state[S_BAD] = 1u;  // (not the list the marks were made from)
        if (at < 3 * n) relseq[at] = v;
        at++;
    }
}
__global__ __launch_bounds__(TB) void k_w_rw_parents(size_t n, const uint32_t* al, const uint32_t* a_ex, const uint32_t* f_ex, const uint32_t* dp,
                                                     const uint32_t* n_ex, const uint32_t* relseq, uint32_t first_fresh, const uint32_t* fifo, uint32_t head,
                                                     uint32_t L, uint32_t cap, uint32_t* state, uint32_t* par, uint32_t* slot) {
    const size_t i = (size_t)blockIdx.x * TB + threadIdx.x;
    if (i >= n || !al[i]) return;
    const uint32_t before = n_ex[i], through = max(before, dp[i]);
    if (through > before) {
        slot[i] = first_fresh + through - 1u;
        return;
    }
    const uint32_t at = a_ex[i] - through;  // A_i - N_i - 1
    if (at < L) {
        slot[i] = fifo[((uint64_t)head + at) % cap];
        return;
    }
    const uint32_t e = at - L < f_ex[i] ? relseq[at - L] : NONE;
    if (e == NONE || e == PIN || (!(e & TAG) && e >= i)) {  // (cannot happen for the list the marks were made from)
        state[S_BAD] = 1u;
        slot[i] = 0u;
    } else if (e & TAG) {
        slot[i] = e & ~TAG;
    } else {
        par[i] = e;
    }
}
__global__ __launch_bounds__(TB) void k_w_jump(uint32_t* par, size_t n, uint32_t* changed) {
    const size_t i = (size_t)blockIdx.x * TB + threadIdx.x;
    if (i >= n) return;
    const uint32_t p = par[i];
    if (p == (uint32_t)i) return;
    const uint32_t pp = par[p];
    if (pp != p) {
        par[i] = pp;
        *changed = 1u;
    }
}
__global__ __launch_bounds__(TB) void k_w_slots(size_t n, const uint32_t* al, const uint32_t* par, uint32_t* slot) {
    const size_t i = (size_t)blockIdx.x * TB + threadIdx.x;
    if (i >= n || !al[i]) return;
    const uint32_t p = par[i];
    if (p != (uint32_t)i) slot[i] = slot[p];
}
// the feed's releases that it did not consume itself, as slot numbers behind the ring's entries (d: which totals of `state`)
__global__ __launch_bounds__(TB) void k_w_rw_append(size_t n, int d, const uint32_t* relseq, const uint32_t* slot, uint32_t* fifo, uint32_t head, uint32_t L,
                                                    uint32_t cap, uint32_t* state) {
    const size_t k = (size_t)blockIdx.x * TB + threadIdx.x;
    const uint64_t ftot = state[S_FTOT_G + d], consumed = (uint64_t)state[S_ATOT_G + d] - state[S_NLOC_G + d];
    if (k >= ftot || k >= 3 * n || L + k < consumed) return;
    if (consumed > L + ftot || L + ftot - consumed > cap) {
        state[S_BAD] = 1u;
        return;
    }
    const uint32_t e = relseq[k];
    uint32_t s = 0u;
    if (e & TAG) s = e & ~TAG;
    else if (e < n) s = slot[e];
    fifo[((uint64_t)head + L + k) % cap] = s;
}
__global__ __launch_bounds__(TB) void k_w_rw_slotof(size_t n, uint32_t W, const uint32_t* sk, const uint32_t* sv, const uint32_t* slot, uint32_t* slotof) {
    const size_t j = (size_t)blockIdx.x * TB + threadIdx.x;
    if (j >= n) return;
    const uint32_t w = sk[j];
    if (w >= W || (j + 1 < n && sk[j + 1] == w)) return;
    slotof[w] = slot[sv[j]];
}
__global__ __launch_bounds__(TB) void k_w_rewrite(const rv_op* ops, size_t n, const uint32_t* pins, const uint32_t* rank, uint32_t Wg, const uint32_t* va,
                                                  const uint32_t* vb, const uint32_t* slot, uint32_t P, uint32_t new_z, uint32_t new_g, rv_op* out) {
    const size_t i = (size_t)blockIdx.x * TB + threadIdx.x;
    if (i >= n) return;
    rv_op op = ops[i];
    auto rank_of = [&](uint32_t w) { return (rank && w < Wg) ? rank[w] : 0u; };
    if (op.domain == RV_DOM_SIZEHINT) {
        op.a = new_z;
        op.b = new_g;
    } else if (op.domain == RV_DOM_B2A) {
        op.a = rank_of(op.a);
        op.dst = slot[i];
    } else if (op.domain <= RV_DOM_Z64) {
        const int d = op.domain == RV_DOM_GF2 ? G : Z;
        const int r = op_reads(op.opcode);
        if (r >= 1) {
            const uint32_t v = va[i];
            op.a = v == PIN ? rank_of(op.a) : v == NONE ? (d == G ? P : 0u) : (v & TAG) ? (v & ~TAG) : slot[v];
        }
        if (r >= 2) {
            const uint32_t v = vb[i];
            op.b = v == PIN ? rank_of(op.b) : v == NONE ? (d == G ? P : 0u) : (v & TAG) ? (v & ~TAG) : slot[v];
        }
        if (op.opcode != RV_OP_ASSERTZERO) op.dst = (d == G && pinned(pins, op.dst, Wg)) ? rank_of(op.dst) : slot[i];
    }
    out[i] = op;
}

}  // namespace

enum class Phase { SCAN, FEED };

struct WinCompactor : WinStage {
    Phase phase = Phase::SCAN;
    uint64_t W[2];                             // counts in force ([G], [Z]): the tables' lengths
    uint32_t* tab[2] = {nullptr, nullptr};     // W[d] words def (the rewrite pass: slotof), then W[d] words rd
    uint32_t *pins = nullptr, *rank = nullptr; // W[G] words each; pins from the first B2A op on, rank from the end of the first scan
    uint32_t* marks = nullptr;
    uint64_t marks_cap = 0;                    // bytes
    uint32_t* fifo[2] = {nullptr, nullptr};
    uint32_t cap[2] = {0, 0}, head[2] = {0, 0}, len[2] = {0, 0}, fresh[2] = {0, 0};
    uint64_t values[2] = {0, 0};
    uint32_t scans = 0;
    bool b2a = false, ops_of[2] = {false, false};
    rv_compact_info info{};

    bool at(Phase ph) const { return !failed && phase == ph; }
    uint32_t* state() const { return (uint32_t*)block; }  // (the block's start)
    uint32_t* def(int d) const { return tab[d]; }
    uint32_t* rd(int d) const { return tab[d] + W[d]; }
    size_t state_bytes() const {
        return WIN_BLOCK_BYTES + 8 * (size_t)(tab[G] ? W[G] : 0) + 8 * (size_t)(tab[Z] ? W[Z] : 0) + (pins ? 4 * (size_t)W[G] : 0) +
               (rank ? 4 * (size_t)W[G] : 0) + (size_t)marks_cap + 4 * (size_t)(fifo[G] ? cap[G] : 0) + 4 * (size_t)(fifo[Z] ? cap[Z] : 0);
    }
};

namespace {

// the tables of domain d at length w (>= the present one), the old contents kept; on an error nothing is held that was not held before
int grow_tables(WinCompactor* c, int d, uint64_t w) {
    if (w == c->W[d] && (c->tab[d] || !w)) return RV_OK;
    uint32_t* t = (uint32_t*)c->take(8 * (size_t)w);
    uint32_t* p = (d == G && c->pins) ? (uint32_t*)c->take(4 * (size_t)w) : nullptr;
    if (!t || (d == G && c->pins && !p)) {
        c->give(t), c->give(p);
        return RV_E_NOMEM;
    }
    const uint64_t old = c->tab[d] ? c->W[d] : 0;
    hipError_t e = hipSuccess;
    if (old) {
        e = hipMemcpyAsync(t, c->tab[d], 4 * old, hipMemcpyDeviceToDevice, c->st);
        if (e == hipSuccess) e = hipMemcpyAsync(t + w, c->tab[d] + old, 4 * old, hipMemcpyDeviceToDevice, c->st);
        if (e == hipSuccess && p) e = hipMemcpyAsync(p, c->pins, 4 * old, hipMemcpyDeviceToDevice, c->st);
    }
    if (e == hipSuccess) e = hipMemsetAsync(t + old, 0xFF, 4 * (w - old), c->st);
    if (e == hipSuccess) e = hipMemsetAsync(t + w + old, 0, 4 * (w - old), c->st);
    if (e == hipSuccess && p) e = hipMemsetAsync(p + old, 0, 4 * (w - old), c->st);
    const hipError_t es = hipStreamSynchronize(c->st);  // (also after an error: the blocks go back to an idle stream)
    if (e != hipSuccess || es != hipSuccess) {
        (void)hipGetLastError();
        c->give(t), c->give(p);
        return RV_E_DEVICE;
    }
    c->give(c->tab[d]);
    c->tab[d] = t, c->W[d] = w;
    if (p) c->give(c->pins), c->pins = p;
    return RV_OK;
}
int grow_marks(WinCompactor* c, uint64_t bytes) {
    if (bytes <= c->marks_cap) return RV_OK;
    const uint64_t want = (bytes + 255) / 256 * 256;
    uint32_t* m = (uint32_t*)c->take(want);
    if (!m) return RV_E_NOMEM;
    hipError_t e = c->marks_cap ? hipMemcpyAsync(m, c->marks, c->marks_cap, hipMemcpyDeviceToDevice, c->st) : hipSuccess;
    if (e == hipSuccess) e = hipMemsetAsync((uint8_t*)m + c->marks_cap, 0, want - c->marks_cap, c->st);
    const hipError_t es = hipStreamSynchronize(c->st);
    if (e != hipSuccess || es != hipSuccess) {
        (void)hipGetLastError();
        c->give(m);
        return RV_E_DEVICE;
    }
    c->give(c->marks);
    c->marks = m, c->marks_cap = want;
    return RV_OK;
}
// the feed's digest sum goes to the block; the feed's words of the state are cleared
hipError_t begin_feed(WinCompactor* c, const rv_op* d_ops, size_t n) {
    uint32_t* state = c->state();
    hipError_t e = hipMemsetAsync(state + S_FEED_FIRST, 0, (S_WORDS - S_FEED_FIRST) * 4, c->st);
    if (e == hipSuccess) e = hipMemsetAsync(state + S_ERR_LO, 0xFF, 8, c->st);
    return e == hipSuccess ? stage_digest(*c, d_ops, n, c->pos) : e;
}
struct FeedWords {
    std::vector<uint32_t> h = std::vector<uint32_t>(S_WORDS);
    uint64_t digest = 0;
};
hipError_t fetch_feed(WinCompactor* c, FeedWords& f) {
    hipError_t e = hipMemcpyAsync(f.h.data(), c->state(), S_WORDS * 4, hipMemcpyDeviceToHost, c->st);
    if (e == hipSuccess) e = stage_fetch_digest(*c, &f.digest);
    if (e == hipSuccess) e = hipStreamSynchronize(c->st);
    return e;
}

int scan_impl(WinCompactor* c, const DevAlloc& CA, const rv_op* ops, size_t n) {
    hipStream_t st = c->st;
    Scratch S(CA, st);
    const uint32_t gb = blocks(n, TB);
    const bool first = c->scans == 0;
    uint32_t *kbuf[2], *vbuf[2];
    for (int k = 0; k < 2; k++) kbuf[k] = S.get<uint32_t>(n), vbuf[k] = S.get<uint32_t>(n);
    uint32_t* last = S.get<uint32_t>(n);
    CDNEED(kbuf[0] && kbuf[1] && vbuf[0] && vbuf[1] && last);
    uint32_t* state = c->state();
    FeedWords f;
    CDCHK(begin_feed(c, ops, n));
    bool dom[2] = {c->W[G] > 0, c->W[Z] > 0};
    if (first) {
        k_pr_hints<<<gb, TB, 0, st>>>(ops, n, kbuf[0], kbuf[1]);
        CDCHK((scan_excl<uint32_t, MaxU32>(S, st, kbuf[0], vbuf[0], n, &state[S_HINT_Z])));
        CDCHK((scan_excl<uint32_t, MaxU32>(S, st, kbuf[1], vbuf[1], n, &state[S_HINT_G])));
        k_w_classify<<<gb, TB, 0, st>>>(ops, n, c->W[Z], c->W[G], vbuf[0], vbuf[1], state);
        CDCHK(hipGetLastError());
        CDCHK(fetch_feed(c, f));
        if (f.h[S_ERR_HI] != 0xFFFFFFFFu || f.h[S_ERR_LO] != 0xFFFFFFFFu) {
            c->failed = true;
            return (int)(f.h[S_ERR_LO] & 0xFFu);
        }
        const uint64_t wz = std::max<uint64_t>(c->W[Z], f.h[S_HINT_Z]), wg = std::max<uint64_t>(c->W[G], f.h[S_HINT_G]);
        if (!stage_wires_ok(wz, wg)) {
            c->failed = true;
            return RV_E_UNSUPPORTED;
        }
        if (f.h[S_B2A] && !c->pins) {
            c->pins = (uint32_t*)c->take(4 * (size_t)c->W[G]);
            CDNEED(c->pins);
            CDCHK(hipMemsetAsync(c->pins, 0, 4 * (size_t)c->W[G], st));
        }
        if (int rc = grow_tables(c, G, wg)) return rc;
        if (int rc = grow_tables(c, Z, wz)) return rc;
        if (int rc = grow_marks(c, c->pos + n)) return rc;
        c->values[G] += f.h[S_VALUES_G], c->values[Z] += f.h[S_VALUES_Z];
        c->b2a = c->b2a || f.h[S_B2A];
        c->ops_of[G] = c->ops_of[G] || f.h[S_OPS_G], c->ops_of[Z] = c->ops_of[Z] || f.h[S_OPS_Z];
        if (f.h[S_B2A]) k_w_pins<<<gb, TB, 0, st>>>(ops, n, c->pins, (uint32_t)c->W[G]);
        dom[G] = f.h[S_OPS_G] != 0, dom[Z] = f.h[S_OPS_Z] != 0;
    }
    const uint32_t* pins = first ? nullptr : c->pins;  // (the first scan of a list with B2A ops is made for the pin table)
    const uint32_t Wg = (uint32_t)c->W[G];
    const uint64_t total = first ? c->pos + n : c->total;
    k_w_own<<<gb, TB, 0, st>>>(ops, n, c->pos, pins, Wg, (uint8_t*)c->marks);
    CDCHK(hipMemsetAsync(last, 0, n * 4, st));
    for (int d = 0; d < 2; d++) {
        if (!dom[d] || !c->W[d]) continue;
        const uint32_t W = (uint32_t)c->W[d];
        k_w_keys<<<gb, TB, 0, st>>>(ops, n, d, W, pins, Wg, kbuf[0], vbuf[0]);
        int which = 0;
        CDCHK(radix_sort(S, st, kbuf, vbuf, n, bit_len(W), &which));
        k_w_scan_reads<<<gb, TB, 0, st>>>(ops, n, c->pos, d, W, kbuf[which], vbuf[which], pins, Wg, c->def(d), c->rd(d), last, state);
        k_w_scan_defs<<<gb, TB, 0, st>>>(n, c->pos, W, kbuf[which], vbuf[which], last, c->def(d), c->rd(d), c->marks, total);
        CDCHK(hipGetLastError());
    }
    if (!first) CDCHK(fetch_feed(c, f));
    else CDCHK(hipStreamSynchronize(st));
    c->digest += f.digest;
    c->pos += n;
    return RV_OK;
}

// steps 4 - 5 of domain d with the carry-in
int rewrite_domain(WinCompactor* c, Scratch& S, const rv_op* ops, size_t n, int d, uint32_t* kbuf[2], uint32_t* vbuf[2], uint32_t* va, uint32_t* vb,
                   uint32_t* par, uint32_t* slot, uint32_t* al, uint32_t* fr, uint32_t* a_ex, uint32_t* f_ex, uint32_t* dp, uint32_t* n_ex, uint32_t* relseq,
                   uint32_t* changed) {
    hipStream_t st = c->st;
    const uint32_t gb = blocks(n, TB), W = (uint32_t)c->W[d], Wg = (uint32_t)c->W[G];
    uint32_t* state = c->state();
    k_w_keys<<<gb, TB, 0, st>>>(ops, n, d, W, c->pins, Wg, kbuf[0], vbuf[0]);
    int which = 0;
    CDCHK(radix_sort(S, st, kbuf, vbuf, n, bit_len(W), &which));
    k_w_rw_reads<<<gb, TB, 0, st>>>(ops, n, d, W, kbuf[which], vbuf[which], c->pins, Wg, c->def(d), va, vb, state);
    k_w_rw_counts<<<gb, TB, 0, st>>>(n, c->pos, d, c->marks, al, fr);
    CDCHK(hipGetLastError());
    CDCHK((scan_excl<uint32_t, SumU32>(S, st, al, a_ex, n, &state[S_ATOT_G + d])));
    CDCHK((scan_excl<uint32_t, SumU32>(S, st, fr, f_ex, n, &state[S_FTOT_G + d])));
    k_w_rw_demand<<<gb, TB, 0, st>>>(al, a_ex, f_ex, n, c->len[d], dp);
    CDCHK((scan_excl<uint32_t, MaxU32>(S, st, dp, n_ex, n, &state[S_NLOC_G + d])));
    k_w_rw_released<<<gb, TB, 0, st>>>(n, c->pos, d, c->marks, va, vb, f_ex, relseq, state);
    const uint32_t base = d == G ? (uint32_t)(c->info.gf2_pinned + c->info.gf2_zero_wire) : c->info.z64_zero_wire;
    k_w_rw_parents<<<gb, TB, 0, st>>>(n, al, a_ex, f_ex, dp, n_ex, relseq, base + c->fresh[d], c->fifo[d], c->head[d], c->len[d], c->cap[d], state, par, slot);
    CDCHK(hipGetLastError());
    CDCHK(hipMemsetAsync(changed, 0, MAX_ROUNDS * 4, st));
    for (int r = 0; r < MAX_ROUNDS; r++) {
        k_w_jump<<<gb, TB, 0, st>>>(par, n, changed + r);
        if (r % ROUNDS_PER_LOOK == ROUNDS_PER_LOOK - 1) {
            uint32_t ch = 0;
            CDCHK(hipMemcpyAsync(&ch, changed + r, 4, hipMemcpyDeviceToHost, st));
            CDCHK(hipStreamSynchronize(st));
            if (!ch) break;
        }
    }
    k_w_slots<<<gb, TB, 0, st>>>(n, al, par, slot);
    k_w_rw_append<<<blocks(3 * n, TB), TB, 0, st>>>(n, d, relseq, slot, c->fifo[d], c->head[d], c->len[d], c->cap[d], state);
    k_w_rw_slotof<<<gb, TB, 0, st>>>(n, W, kbuf[which], vbuf[which], slot, c->def(d));
    CDCHK(hipGetLastError());
    return RV_OK;
}

int feed_impl(WinCompactor* c, const DevAlloc& CA, const rv_op* ops, size_t n, rv_op* out) {
    hipStream_t st = c->st;
    Scratch S(CA, st);
    const uint32_t gb = blocks(n, TB);
    uint32_t *kbuf[2], *vbuf[2];
    for (int k = 0; k < 2; k++) kbuf[k] = S.get<uint32_t>(n), vbuf[k] = S.get<uint32_t>(n);
    uint32_t *va = S.get<uint32_t>(n), *vb = S.get<uint32_t>(n), *par = S.get<uint32_t>(n), *slot = S.get<uint32_t>(n);
    uint32_t *al = S.get<uint32_t>(n), *fr = S.get<uint32_t>(n), *a_ex = S.get<uint32_t>(n), *f_ex = S.get<uint32_t>(n), *dp = S.get<uint32_t>(n);
    uint32_t *n_ex = S.get<uint32_t>(n), *relseq = S.get<uint32_t>(3 * n), *changed = S.get<uint32_t>(MAX_ROUNDS);
    CDNEED(kbuf[0] && kbuf[1] && vbuf[0] && vbuf[1] && va && vb && par && slot && al && fr && a_ex && f_ex && dp && n_ex && relseq && changed);
    CDCHK(begin_feed(c, ops, n));
    CDCHK(hipMemsetAsync(va, 0xFF, n * 4, st));
    CDCHK(hipMemsetAsync(vb, 0xFF, n * 4, st));
    CDCHK(hipMemsetAsync(slot, 0, n * 4, st));
    k_w_iota<<<gb, TB, 0, st>>>(par, n);
    CDCHK(hipGetLastError());
    for (int d = 0; d < 2; d++)
        if (c->ops_of[d] && c->W[d])
            if (int rc = rewrite_domain(c, S, ops, n, d, kbuf, vbuf, va, vb, par, slot, al, fr, a_ex, f_ex, dp, n_ex, relseq, changed)) return rc;
    FeedWords f;
    CDCHK(fetch_feed(c, f));  // (before the records are written: a feed that is not the scanned list writes nothing)
    bool bad = f.h[S_BAD] != 0;
    uint32_t consumed[2] = {0, 0};
    for (int d = 0; d < 2 && !bad; d++) {
        if (f.h[S_NLOC_G + d] > f.h[S_ATOT_G + d]) bad = true;
        else consumed[d] = f.h[S_ATOT_G + d] - f.h[S_NLOC_G + d];
        if (!bad && ((uint64_t)consumed[d] > (uint64_t)c->len[d] + f.h[S_FTOT_G + d] || (uint64_t)c->fresh[d] + f.h[S_NLOC_G + d] > c->cap[d])) bad = true;
    }
    if (bad) {
        c->failed = true;
        return RV_E_ARG;
    }
    k_w_rewrite<<<gb, TB, 0, st>>>(ops, n, c->pins, c->rank, (uint32_t)c->W[G], va, vb, slot, (uint32_t)c->info.gf2_pinned, (uint32_t)c->info.z64_wires,
                                   (uint32_t)c->info.gf2_wires, out);
    CDCHK(hipGetLastError());
    CDCHK(hipStreamSynchronize(st));
    for (int d = 0; d < 2; d++) {
        if (!c->cap[d]) continue;
        c->head[d] = (uint32_t)(((uint64_t)c->head[d] + consumed[d]) % c->cap[d]);
        c->len[d] = c->len[d] + f.h[S_FTOT_G + d] - consumed[d];
        c->fresh[d] += f.h[S_NLOC_G + d];
    }
    c->digest += f.digest;
    c->pos += n;
    return RV_OK;
}

int reset_rewrite(WinCompactor* c) {
    hipError_t e = hipSuccess;
    for (int d = 0; d < 2; d++) {
        if (e == hipSuccess && c->tab[d] && c->W[d]) e = hipMemsetAsync(c->def(d), 0xFF, 4 * (size_t)c->W[d], c->st);
        c->head[d] = c->len[d] = c->fresh[d] = 0;
    }
    if (e != hipSuccess || hipStreamSynchronize(c->st) != hipSuccess) {
        (void)hipGetLastError();
        return RV_E_DEVICE;
    }
    c->pos = 0, c->digest = 0;
    return RV_OK;
}

int scan_end_impl(WinCompactor* c, const DevAlloc& CA, int* again, rv_compact_info* info) {
    hipStream_t st = c->st;
    uint32_t* state = c->state();
    if (c->scans == 0) c->total = c->pos, c->digest0 = c->digest;
    if (c->scans == 0 && c->b2a) {  // the pins are complete: their ranks, and the marks from a second scan
        Scratch S(CA, st);
        uint32_t* rank = (uint32_t*)c->take(4 * (size_t)c->W[G]);
        CDNEED(rank);
        c->rank = rank;
        CDCHK((scan_excl<uint32_t, SumU32>(S, st, c->pins, c->rank, (size_t)c->W[G], &state[S_P])));
        if (c->marks_cap) CDCHK(hipMemsetAsync(c->marks, 0, c->marks_cap, st));
        for (int d = 0; d < 2; d++) {
            if (!c->tab[d] || !c->W[d]) continue;
            CDCHK(hipMemsetAsync(c->def(d), 0xFF, 4 * (size_t)c->W[d], st));
            CDCHK(hipMemsetAsync(c->rd(d), 0, 4 * (size_t)c->W[d], st));
        }
        CDCHK(hipMemsetAsync(state + S_ZERO_G, 0, 8, st));
        CDCHK(hipStreamSynchronize(st));
        c->scans = 1, c->pos = 0, c->digest = 0;
        *again = 1;
        return RV_OK;
    }
    Scratch S(CA, st);
    for (int d = 0; d < 2; d++)
        if (c->tab[d] && c->W[d]) k_w_scan_rest<<<blocks((size_t)c->W[d], TB), TB, 0, st>>>((uint32_t)c->W[d], c->def(d), c->rd(d), c->marks, c->total);
    CDCHK(hipGetLastError());
    const size_t nb = (size_t)((c->total + RB - 1) / RB);
    std::vector<int32_t> parts(nb * 6);
    if (nb) {
        int32_t* d_parts = S.get<int32_t>(nb * 6);
        CDNEED(d_parts);
        k_w_marks_reduce<<<(uint32_t)nb, RB, 0, st>>>(c->marks, c->total, d_parts);
        CDCHK(hipGetLastError());
        CDCHK(fetch(st, parts, d_parts));
    }
    std::vector<uint32_t> h(S_WORDS);
    CDCHK(fetch(st, h, state));
    CDCHK(hipStreamSynchronize(st));
    if (h[S_BAD]) {
        c->failed = true;
        return RV_E_ARG;
    }
    int64_t A[2] = {0, 0}, F[2] = {0, 0}, N[2] = {0, 0};
    for (size_t b = 0; b < nb; b++)
        for (int d = 0; d < 2; d++) {
            const int32_t* p = &parts[(b * 2 + d) * 3];
            if (p[0]) N[d] = std::max<int64_t>(N[d], A[d] - F[d] + p[2]);
            A[d] += p[0], F[d] += p[1];
        }
    rv_compact_info ci{};
    ci.gf2_pinned = c->b2a ? h[S_P] : 0, ci.gf2_zero_wire = h[S_ZERO_G], ci.z64_zero_wire = h[S_ZERO_Z];
    ci.z64_wires = (uint64_t)h[S_ZERO_Z] + (uint64_t)N[Z], ci.gf2_wires = ci.gf2_pinned + h[S_ZERO_G] + (uint64_t)N[G];
    ci.gf2_values = c->values[G], ci.z64_values = c->values[Z];
    if (ci.z64_wires >= MAX_SLOTS || ci.gf2_wires >= MAX_SLOTS) {
        c->failed = true;
        return RV_E_UNSUPPORTED;
    }
    for (int d = 0; d < 2; d++) {
        c->cap[d] = (uint32_t)std::max<int64_t>(N[d], 1);
        c->fifo[d] = N[d] ? (uint32_t*)c->take(4 * (size_t)c->cap[d]) : nullptr;
        CDNEED(!N[d] || c->fifo[d]);
    }
    c->info = ci;
    c->scans++;
    if (int rc = reset_rewrite(c)) return rc;
    c->phase = Phase::FEED;
    *again = 0;
    if (info) *info = ci;
    return RV_OK;
}
#undef CDCHK
#undef CDNEED

// a compactor that closes drops its rings
int settled(WinCompactor* c, int rc) {
    return stage_settled(*c, rc, [c] {
        for (int d = 0; d < 2; d++) c->give(c->fifo[d]), c->fifo[d] = nullptr;
    });
}

}  // namespace

int wincompact_begin(hipStream_t st, const DevAlloc& A, uint64_t z64_wires, uint64_t gf2_wires, WinCompactor** out) {
    if (!stage_wires_ok(z64_wires, gf2_wires)) return RV_E_UNSUPPORTED;
    WinCompactor* c = new WinCompactor;
    c->W[G] = 0, c->W[Z] = 0;
    int rc = stage_open(*c, st, A);
    if (rc == RV_OK) rc = grow_tables(c, G, gf2_wires);
    if (rc == RV_OK) rc = grow_tables(c, Z, z64_wires);
    if (rc != RV_OK) {
        wincompact_destroy(c);
        return rc;
    }
    *out = c;
    return RV_OK;
}

int wincompact_admit_scan(WinCompactor* c, size_t n) {
    if (!c->at(Phase::SCAN)) return RV_E_ARG;
    if (c->scans && n < WIN_INDEX_LIMIT) return c->pos + n > c->total ? RV_E_ARG : RV_OK;
    return stage_admit_first(*c, n);
}
int wincompact_admit_feed(const WinCompactor* c, size_t n) {
    if (!c->at(Phase::FEED)) return RV_E_ARG;
    if (n >= WIN_INDEX_LIMIT) return RV_E_UNSUPPORTED;
    return c->pos + n > c->total ? RV_E_ARG : RV_OK;
}

int wincompact_scan(WinCompactor* c, const rv_op* d_ops, size_t n, size_t upload_bytes) {
    if (int rc = wincompact_admit_scan(c, n)) return rc;
    if (!n) return RV_OK;
    return settled(c, stage_counted(*c, upload_bytes, [&](const DevAlloc& CA) { return scan_impl(c, CA, d_ops, n); }));
}

int wincompact_scan_end(WinCompactor* c, int* again, rv_compact_info* info) {
    if (!c->at(Phase::SCAN) || !again) return RV_E_ARG;
    if (c->scans && !stage_pass_done(*c)) return RV_E_ARG;
    return settled(c, stage_counted(*c, 0, [&](const DevAlloc& CA) { return scan_end_impl(c, CA, again, info); }));
}

int wincompact_feed(WinCompactor* c, const rv_op* d_ops, size_t n, rv_op* d_out, size_t upload_bytes) {
    if (int rc = wincompact_admit_feed(c, n)) return rc;
    if (n)
        if (int rc = settled(c, stage_counted(*c, upload_bytes, [&](const DevAlloc& CA) { return feed_impl(c, CA, d_ops, n, d_out); }))) return rc;
    if (c->pos == c->total && !stage_pass_done(*c)) return RV_E_ARG;  // (the pass was not the scanned list)
    return RV_OK;
}

int wincompact_rewind(WinCompactor* c) {
    if (!c->at(Phase::FEED) || c->pos != c->total) return RV_E_ARG;
    return settled(c, reset_rewrite(c));
}

int wincompact_info(const WinCompactor* c, rv_compactor_info* info) {
    if (c->failed) return RV_E_ARG;
    *info = rv_compactor_info{};
    info->total_ops = c->scans ? c->total : c->pos;
    info->state_bytes = c->state_bytes();
    info->peak_feed_bytes = c->peak_feed;
    info->scans = c->scans;
    info->b2a = c->b2a ? 1u : 0u;
    return RV_OK;
}

void wincompact_destroy(WinCompactor* c) {
    if (!c) return;
    stage_close(*c);
    for (int d = 0; d < 2; d++) c->give(c->tab[d]), c->give(c->fifo[d]);
    c->give(c->pins), c->give(c->rank), c->give(c->marks);
    delete c;
}

}  // namespace rv
