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

// ---- the emit: a tile of PRUNE_TILE input records gathers its kept ones into an image that lies in LDS at the position modulo 16
// its bytes have in d_out (link.h's layout).  `first` kept records precede the tile's. ----
PR_HD inline uint32_t pr_image_shift(uint64_t out_addr, uint64_t first) { return (uint32_t)((out_addr + first * 24) & 15u); }
PR_HD inline uint32_t pr_chunk(uint32_t c, uint32_t sh, uint32_t span) { return lk_chunk(c, sh, span); }

}  // namespace rv
