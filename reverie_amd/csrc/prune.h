// Ops no assertion or output depends on, dropped: on the host (rv_ops_prune, prune.cpp) and on the GPU (prune_dev.hip).  The rule is in
// include/reverie_amd.h, the steps in DESIGN §23 and at the head of prune_dev.hip.
//
// ONE RECORD'S PART IN THE RULE -- the value it defines (pr_def), what it reads (pr_n_reads, pr_read), whether it is a root
// (pr_root), the class it is counted in when it is dropped (pr_class), compile_ops' check of it (pr_check) -- is decided here and
// nowhere else, and so are the search that resolves a read (pr_value_read) and the way a tile's image is cut into stores (pr_chunk,
// link.h's lk_chunk: records are 24 bytes and buffers 8-byte aligned here too).  The host sweep, the kernels and the CPU model of
// tests/prune_model.cpp all call these functions.
//
// Everything here is plain C++ (the CPU model compiles it with g++); prune_dev.h holds what needs HIP.
#pragma once
#include <stdint.h>

#include "link.h"

#define PR_HD LK_HD

namespace rv {

constexpr uint32_t PR_NONE = 0xFFFFFFFFu;  // a read of an index no op wrote: the zero wire; no value
constexpr int PR_G = 0, PR_Z = 1;          // the domains, as array indices
// records per workgroup of the emit kernel, and its LDS image: the shift, the records, the last chunk's other half
constexpr uint32_t PRUNE_TILE = LINK_TILE;
constexpr uint32_t PR_IMAGE = LK_IMAGE;
// the classes of rv_prune_info, in its order: dropped ops first, then the Inputs kept unread
enum { PR_C_MUL_G, PR_C_MUL_Z, PR_C_B2A, PR_C_RANDOM_G, PR_C_RANDOM_Z, PR_C_OTHER_G, PR_C_OTHER_Z, PR_C_INPUT_G, PR_C_INPUT_Z, PR_CLASSES };

// the domain of the value the record defines (-1: it defines none).  Nothing is pinned: a B2A defines a Z64 value, every GF(2) write
// is a writer like any other.
PR_HD inline int pr_def(const rv_op& op) {
    if (op.domain == RV_DOM_B2A) return PR_Z;
    if (op.domain > RV_DOM_Z64 || op.opcode == RV_OP_ASSERTZERO) return -1;
    return op.domain == RV_DOM_GF2 ? PR_G : PR_Z;
}
// the domain its reads lie in (meaningful where pr_n_reads is not 0)
PR_HD inline int pr_read_dom(const rv_op& op) { return op.domain == RV_DOM_Z64 ? PR_Z : PR_G; }
// how many indices it reads: a B2A the 64 GF(2) indices a .. a + 63
PR_HD inline uint32_t pr_n_reads(const rv_op& op) {
    if (op.domain == RV_DOM_B2A) return 64;
    if (op.domain > RV_DOM_Z64) return 0;
    const uint32_t f = lk_fields(op.opcode);
    return (f & LK_A ? 1u : 0u) + (f & LK_B ? 1u : 0u);
}
PR_HD inline uint32_t pr_read(const rv_op& op, uint32_t k) { return op.domain == RV_DOM_B2A ? op.a + k : k ? op.b : op.a; }
PR_HD inline bool pr_is_input(const rv_op& op) { return op.domain <= RV_DOM_Z64 && op.opcode == RV_OP_INPUT; }
// a root is kept whatever reads it: AssertZero, Input (witness order and length stay), SizeHint (it stays in place)
PR_HD inline bool pr_root(const rv_op& op) {
    return op.domain == RV_DOM_SIZEHINT || (op.domain <= RV_DOM_Z64 && (op.opcode == RV_OP_ASSERTZERO || op.opcode == RV_OP_INPUT));
}
// the class a dropped record is counted in (one that is no root)
PR_HD inline int pr_class(const rv_op& op) {
    if (op.domain == RV_DOM_B2A) return PR_C_B2A;
    const int z = op.domain == RV_DOM_Z64 ? 1 : 0;
    if (op.opcode == RV_OP_MUL) return PR_C_MUL_G + z;
    if (op.opcode == RV_OP_RANDOM) return PR_C_RANDOM_G + z;
    return PR_C_OTHER_G + z;
}

// compile_ops' checks of one record against the counts in force at it (nz, ng: a SizeHint's fields already count) -> RV_OK,
// RV_E_BAD_OP or RV_E_WIRE_OOB
PR_HD inline int pr_check(const rv_op& op, uint64_t nz, uint64_t ng) {
    if (op.reserved != 0) return RV_E_BAD_OP;
    if (op.domain == RV_DOM_SIZEHINT) return RV_OK;
    if (op.domain == RV_DOM_B2A) return (op.dst >= nz || (uint64_t)op.a + 64 > ng) ? RV_E_WIRE_OOB : RV_OK;
    if (op.domain > RV_DOM_Z64 || op.opcode > RV_OP_CONST) return RV_E_BAD_OP;
    const uint64_t n = op.domain == RV_DOM_GF2 ? ng : nz;
    const uint32_t f = lk_fields(op.opcode);
    if (((f & LK_DST) && op.dst >= n) || ((f & LK_A) && op.a >= n) || ((f & LK_B) && op.b >= n)) return RV_E_WIRE_OOB;
    return RV_OK;
}

// The value on index w that op i reads: the last pair (w, j) with j < i of one domain's (index, op) pairs sorted by index, then op --
// PR_NONE where no earlier op wrote w.  i = PR_NONE asks for the value w ends on (an output).  Pairs with keys above every index (the
// ops that define nothing in the domain) may follow.
PR_HD inline uint32_t pr_value_read(const uint32_t* sk, const uint32_t* sv, uint32_t n, uint32_t w, uint32_t i) {
    uint32_t lo = 0, hi = n;
    while (lo < hi) {  // (at most 32 steps)
        const uint32_t mid = lo + (hi - lo) / 2;
        const uint32_t k = sk[mid];
        if (k < w || (k == w && sv[mid] < i)) lo = mid + 1;
        else hi = mid;
    }
    return (lo > 0 && sk[lo - 1] == w) ? sv[lo - 1] : PR_NONE;
}

// ---- the window step: the rule on ops [lo, hi) of a list that passes through in windows, from the last window to the
// first.  What a window hears from the ones behind it is one needed byte per index and domain: a kept op behind `hi` reads the value
// now on the index.  The host form is the backward sweep itself; the device form counts and peels as the whole-list call does, with
// the three decisions below around it. ----

// a needed table over memory the caller holds, one byte per index (the host sweep's other table, a hash set, is prune.cpp's)
struct PrDense {
    uint8_t* p;
    void set(uint32_t w) { p[w] = 1; }
    // the flag, cleared
    bool take(uint32_t w) {
        const bool was = p[w] != 0;
        p[w] = 0;
        return was;
    }
};
// The backward sweep over one window: need[PR_G], need[PR_Z] come in as they stand at the window's end and go out as they stand at
// its beginning; keep[i] for the window's n ops; the dropped ops and the Inputs kept unwanted are added to cls[PR_CLASSES].  A
// defining op takes (clears) the flag of its index whether it is kept or not, a kept op then sets the flags of what it reads: every
// index the window writes is killed, and what a kept op reads ahead of the window's writers of it is generated after that.
// -> the ops kept
template <class Need>
inline uint64_t pr_window_sweep(const rv_op* ops, size_t n, Need need[2], uint8_t* keep, uint64_t* cls) {
    uint64_t n_kept = 0;
    for (size_t i = n; i-- > 0;) {
        const rv_op& op = ops[i];
        const int d = pr_def(op);
        const bool wanted = d >= 0 && need[d].take(op.dst);
        const bool kept = wanted || pr_root(op);
        keep[i] = kept;
        if (kept) {
            n_kept++;
            if (pr_is_input(op) && !wanted) cls[PR_C_INPUT_G + d]++;
            const uint32_t r = pr_n_reads(op);
            const int rd = pr_read_dom(op);
            for (uint32_t k = 0; k < r; k++) need[rd].set(pr_read(op, k));
        } else {
            cls[pr_class(op)]++;
        }
    }
    return n_kept;
}

// The device's three decisions, on one domain's sorted (index, op) pairs of the window (nd defining ops) and its needed bytes N
// (W of them).  Pair j is the window's LAST writer of its index when the next pair has another key.
PR_HD inline bool pr_run_last(const uint32_t* sk, uint32_t nd, uint32_t j) { return j + 1 >= nd || sk[j + 1] != sk[j]; }
// live-out: the value pair j's op defines is read behind the window (one more on its count) -- the last writer of a needed index
PR_HD inline bool pr_live_out(const uint32_t* sk, uint32_t nd, uint32_t j, const uint8_t* N, uint64_t W) {
    return pr_run_last(sk, nd, j) && sk[j] < W && N[sk[j]] != 0;
}
// kill: every index the window writes, whoever wrote it, kept or dropped (once per index: by the run's last pair)
PR_HD inline void pr_kill(const uint32_t* sk, uint32_t nd, uint32_t j, uint8_t* N, uint64_t W) {
    if (pr_run_last(sk, nd, j) && sk[j] < W) N[sk[j]] = 0;
}
// gen, after every kill: read k of the kept op i escapes the window (no writer of the index inside it and before i) -> the index is
// needed ahead of the window.  Threads that store to one byte store the same value.
PR_HD inline void pr_gen(const rv_op& op, uint32_t i, uint32_t k, const uint32_t* sk, const uint32_t* sv, uint32_t nd, uint8_t* N, uint64_t W) {
    const uint32_t w = pr_read(op, k);
    if (w < W && pr_value_read(sk, sv, nd, w, i) == PR_NONE) N[w] = 1;
}

// ---- the emit: a tile of PRUNE_TILE input records gathers its kept ones into an image that lies in LDS at the position modulo 16
// its bytes have in d_out (link.h's layout).  `first` kept records precede the tile's. ----
PR_HD inline uint32_t pr_image_shift(uint64_t out_addr, uint64_t first) { return (uint32_t)((out_addr + first * 24) & 15u); }
PR_HD inline uint32_t pr_chunk(uint32_t c, uint32_t sh, uint32_t span) { return lk_chunk(c, sh, span); }

}  // namespace rv
