// Constants folded in op lists: on the host (rv_ops_fold, fold.cpp) and on the GPU (fold_dev.hip).  The rule is in
// include/reverie_amd.h, the steps in DESIGN §24 and at the head of fold_dev.hip.
//
// ONE RECORD'S PART IN THE RULE -- whether it is known given what is known of its reads (fd_known; before anything is propagated:
// given the reads that have no producer -- fd_seed is that for a list that stands alone), the value of a known record (fd_eval, fd_b2a_bit), the record that replaces it (fd_rewrite) and the
// class it is counted in (fd_class) -- is decided here and nowhere else.  What a record defines and reads, compile_ops' check of it,
// the search that resolves a read and the way a tile's image is cut into stores are prune.h's.  The host sweep, the kernels and the
// CPU model of tests/fold_model.cpp all call these functions.
//
// Everything here is plain C++ (the CPU model compiles it with g++); fold_dev.h holds what needs HIP.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "prune.h"

namespace rv {

// records per workgroup of the rewrite kernel, and its LDS image (prune.h's: the shift, the records, the last chunk's other half)
constexpr uint32_t FOLD_TILE = PRUNE_TILE;
// the classes of rv_fold_info, in its order: the rewritten records first, then the assertions of a known value
enum { FD_C_MUL_CONST_G, FD_C_MUL_CONST_Z, FD_C_MUL_LIN_G, FD_C_MUL_LIN_Z, FD_C_B2A, FD_C_OTHER_G, FD_C_OTHER_Z, FD_C_ASSERT_ZERO, FD_C_ASSERT_NONZERO,
       FD_CLASSES, FD_REWRITTEN = FD_C_OTHER_Z + 1 };

// a GF(2) or Z64 record whose opcode is `opc`
PR_HD inline bool fd_is(const rv_op& op, uint32_t opc) { return op.domain <= RV_DOM_Z64 && op.opcode == opc; }
// the constant of an AddConst, SubConst, MulConst or Const as the evaluator takes it (GF(2): bit 0)
PR_HD inline uint64_t fd_imm(const rv_op& op) { return op.domain == RV_DOM_GF2 ? op.imm & 1u : op.imm; }
// a Mul: the one op that a single known read (a zero) makes known
PR_HD inline bool fd_zero_kills(const rv_op& op) { return fd_is(op, RV_OP_MUL); }

// Is the defining record known, given which of its pr_n_reads reads are known (kn[k]) and, for a Mul, their values (v[0], v[1];
// looked at only where kn says known)?  Input and Random never are.
PR_HD inline bool fd_known(const rv_op& op, const bool* kn, const uint64_t* v) {
    if (pr_def(op) < 0) return false;
    if (op.domain == RV_DOM_B2A) {
        bool all = true;
        for (uint32_t k = 0; k < 64; k++) all = all && kn[k];
        return all;
    }
    switch (op.opcode) {
        case RV_OP_CONST: return true;
        case RV_OP_ADD:
        case RV_OP_SUB: return kn[0] && kn[1];
        case RV_OP_MUL: return (kn[0] && kn[1]) || (kn[0] && v[0] == 0) || (kn[1] && v[1] == 0);
        case RV_OP_ADDCONST:
        case RV_OP_SUBCONST: return kn[0];
        case RV_OP_MULCONST: return kn[0] || fd_imm(op) == 0;
        default: return false;  // Input, Random
    }
}
// Is it known before any propagation, in a list that stands alone?  unwritten[k]: read k names an index no earlier op wrote (the
// zero wire, known 0).  This is fd_known with the values 0: the seed kernel calls fd_known itself, with the values a window's
// tables hold for such reads (null tables: 0, this function), and the CPU model of the whole-list call keeps this form.
PR_HD inline bool fd_seed(const rv_op& op, const bool* unwritten) {
    const uint64_t zero[2] = {0, 0};
    return fd_known(op, unwritten, zero);
}
// The value of a known GF(2) or Z64 record from the values of its reads (v[0], v[1]; 0 where a read is not known: a Mul known by a
// zero operand comes out 0 then).  GF(2) values are 0 or 1, Z64 values wrap.
PR_HD inline uint64_t fd_eval(const rv_op& op, const uint64_t* v) {
    const bool g = op.domain == RV_DOM_GF2;
    const uint64_t c = fd_imm(op);
    switch (op.opcode) {
        case RV_OP_CONST: return c;
        case RV_OP_ADD: return g ? v[0] ^ v[1] : v[0] + v[1];
        case RV_OP_SUB: return g ? v[0] ^ v[1] : v[0] - v[1];
        case RV_OP_MUL: return g ? v[0] & v[1] : v[0] * v[1];
        case RV_OP_ADDCONST: return g ? v[0] ^ c : v[0] + c;
        case RV_OP_SUBCONST: return g ? v[0] ^ c : v[0] - c;
        case RV_OP_MULCONST: return g ? v[0] & c : v[0] * c;
        default: return 0;
    }
}
// bit k of a known B2A's value, from the value on index a + k
PR_HD inline uint64_t fd_b2a_bit(uint32_t k, uint64_t bit) { return (bit & 1u) << k; }

PR_HD inline rv_op fd_make(int dom, uint32_t opc, uint32_t dst, uint32_t a, uint64_t imm) {
    rv_op o = {};
    o.domain = (uint8_t)(dom == PR_G ? RV_DOM_GF2 : RV_DOM_Z64), o.opcode = (uint8_t)opc;
    o.dst = dst, o.a = a, o.imm = imm;
    return o;
}
// The record that replaces `op`.  known, val: is the value it defines known, and its value (fd_known, fd_eval; a B2A's 64 reads are
// the caller's to look at); kn, v: its first two reads (not looked at for a B2A).  A record that is not rewritten comes back as it is.
PR_HD inline rv_op fd_rewrite(const rv_op& op, bool known, uint64_t val, const bool* kn, const uint64_t* v) {
    const int d = pr_def(op);
    if (d < 0 || fd_is(op, RV_OP_CONST)) return op;
    if (known) return fd_make(d, RV_OP_CONST, op.dst, 0, val);
    if (op.domain == RV_DOM_B2A) return op;
    const bool only_a = kn[0] && !kn[1], only_b = kn[1] && !kn[0];
    switch (op.opcode) {
        case RV_OP_ADD:
            if (only_a) return fd_make(d, RV_OP_ADDCONST, op.dst, op.b, v[0]);
            if (only_b) return fd_make(d, RV_OP_ADDCONST, op.dst, op.a, v[1]);
            return op;
        case RV_OP_SUB:
            if (only_b) return fd_make(d, RV_OP_SUBCONST, op.dst, op.a, v[1]);
            if (only_a && d == PR_G) return fd_make(d, RV_OP_ADDCONST, op.dst, op.b, v[0]);
            return op;  // Z64 c - x: no single op computes it
        case RV_OP_MUL:  // (a known 0 made the record known)
            if (only_a) return fd_make(d, RV_OP_MULCONST, op.dst, op.b, v[0]);
            if (only_b) return fd_make(d, RV_OP_MULCONST, op.dst, op.a, v[1]);
            return op;
        default: return op;
    }
}
// The class the record counts in, from what fd_rewrite made of it (`now`): -1 where it counts in none.  An AssertZero counts by its
// read (kn[0], v[0]).
PR_HD inline int fd_class(const rv_op& op, const rv_op& now, const bool* kn, const uint64_t* v) {
    if (fd_is(op, RV_OP_ASSERTZERO)) return !kn[0] ? -1 : v[0] == 0 ? FD_C_ASSERT_ZERO : FD_C_ASSERT_NONZERO;
    if (now.domain == op.domain && now.opcode == op.opcode) return -1;
    if (op.domain == RV_DOM_B2A) return FD_C_B2A;
    const int z = op.domain == RV_DOM_Z64 ? 1 : 0;
    if (op.opcode == RV_OP_MUL) return (now.opcode == RV_OP_CONST ? FD_C_MUL_CONST_G : FD_C_MUL_LIN_G) + z;
    return FD_C_OTHER_G + z;
}

// ---- the window step: the rule on ops [lo, hi) of a list that passes through in windows, from the first window to
// the last.  What a window hears from the ones before it is one KNOWN byte and one VALUE word per index and domain: the state of the
// last value defined on the index ahead of the window (nothing written yet: known 0, the zero wire).  The host form is the forward
// sweep itself; the device form seeds and propagates as the whole-list call does, with an escaping read taken from the tables and
// the decisions below around it. ----

// a known table over memory the caller holds, one byte and one word per index (the host sweep's other table, a hash map, is fold.cpp's)
struct FdDense {
    uint8_t* k;
    uint64_t* v;
    bool get(uint32_t w, uint64_t* val) const {
        *val = v[w];
        return k[w] != 0;
    }
    void set(uint32_t w, bool known, uint64_t val) { k[w] = known ? 1 : 0, v[w] = known ? val : 0; }
};
// The forward sweep over n valid records with the state as it stands before them (st[PR_G], st[PR_Z]); the state goes out as it
// stands behind them.  out (may be null, may be ops) receives record j's replacement at j; the counts are added to cls[FD_CLASSES]
// and *n_known.
template <class Known>
inline void fd_window_sweep(const rv_op* ops, size_t n, Known st[2], rv_op* out, uint64_t* cls, uint64_t* n_known) {
    for (size_t i = 0; i < n; i++) {
        const rv_op op = ops[i];  // (a copy: out may be ops)
        const uint32_t r = pr_n_reads(op);
        const int rd = pr_read_dom(op), d = pr_def(op);
        bool kn[64] = {};
        uint64_t v[64] = {};
        for (uint32_t k = 0; k < r; k++) {
            kn[k] = st[rd].get(pr_read(op, k), &v[k]);
            if (!kn[k]) v[k] = 0;
        }
        const bool known = fd_known(op, kn, v);
        uint64_t val = 0;
        if (known && op.domain == RV_DOM_B2A)
            for (uint32_t k = 0; k < 64; k++) val |= fd_b2a_bit(k, v[k]);
        else if (known)
            val = fd_eval(op, v);
        const rv_op now = fd_rewrite(op, known, val, kn, v);
        const int c = fd_class(op, now, kn, v);
        if (c >= 0) cls[c]++;
        if (known) (*n_known)++;
        if (d >= 0) st[d].set(op.dst, known, val);
        if (out) out[i] = now;
    }
}
// fd_window_sweep over tables the caller holds (fold.cpp; K, V: [PR_G], [PR_Z]) -- the fall-back of one windowed device feed
void fold_window_dense(const rv_op* ops, size_t n, uint8_t* const K[2], uint64_t* const V[2], rv_op* out, uint64_t* cls, uint64_t* n_known);
// was the record rewritten (it counts in one of the FD_REWRITTEN classes): fd_rewrite changes the opcode or the domain, or nothing
PR_HD inline bool fd_changed(const rv_op& op, const rv_op& now) { return now.domain != op.domain || now.opcode != op.opcode; }

// The device's decisions around the whole-list steps, on one domain's sorted (index, op) pairs of the window (prune.h's pr_run_last:
// pair j is the window's LAST writer of its index when the next pair has another key).
// table update, after the rewrite has read the tables: the last writer's (known, value) goes to its index -- one storing thread per
// index, no atomics
PR_HD inline void fd_table_update(const uint32_t* sk, const uint32_t* sv, uint32_t nd, uint32_t j, const uint32_t* known, const uint64_t* val, uint8_t* K,
                                  uint64_t* V, uint64_t W) {
    if (!pr_run_last(sk, nd, j) || sk[j] >= W) return;
    const bool kn = known[sv[j]] != 0u;
    K[sk[j]] = kn ? 1 : 0, V[sk[j]] = kn ? val[sv[j]] : 0ull;
}
// replay: the first log entry whose ordinal is not below `ordinal` (the log is ascending by ordinal)
PR_HD inline uint32_t fd_log_lower_bound(const uint32_t* ord, uint32_t n, uint64_t ordinal) {
    uint32_t lo = 0, hi = n;
    while (lo < hi) {
        const uint32_t mid = lo + (hi - lo) / 2;
        if (ord[mid] < ordinal) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

}  // namespace rv
