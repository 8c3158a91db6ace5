// Programs linked from circuit blocks: on the host (rv_link, link.cpp), on the GPU (link_dev.hip) and in windows (rv_link_plan_emit).
// The rule and the order of decisions are in include/reverie_amd.h, the stages in DESIGN §22 and at the head of link_dev.hip.
//
// ONE RECORD'S FATE -- which of its fields name a wire (lk_fields), its code inside a block (lk_judge), inside head or tail
// (lk_malformed), and the record an instance emits for it (lk_rewrite) -- is decided here and nowhere else, and so are the two
// searches of the emit kernel (lk_last_le, lk_gallop) and the way a tile's image is cut into stores (lk_chunk): the host function,
// the kernels and the CPU model of tests/link_model.cpp all call these functions.
//
// Everything up to the `rv` functions at the end is plain C++ (no HIP header is needed: the CPU model compiles it with g++).
#pragma once
#include <stdint.h>

#include "../../include/reverie_amd.h"

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define LK_HD __host__ __device__
#else
#define LK_HD
#endif

namespace rv {

// records per workgroup of the emit kernel (rv_hook_link_tiles reports it)
constexpr uint32_t LINK_TILE = 256;
// items per workgroup of the scans over the Input flags and the instances
constexpr uint32_t LINK_SCAN_BLOCK = 2048;
constexpr uint64_t LK_NO_ERR = ~0ull;
// the limits of decision (1): instances, and block records in all
constexpr uint64_t LK_MAX_INSTANCES = 1ull << 31, LK_MAX_BLOCK_OPS = 1ull << 32;
// records of one emit call
constexpr uint64_t LK_MAX_EMIT = 1ull << 28;

// A record as three 64-bit words: domain | opcode << 8 | reserved << 16 | dst << 32, a | b << 32, imm.
LK_HD inline uint32_t lk_dom(uint64_t w0) { return (uint32_t)w0 & 255u; }
LK_HD inline uint32_t lk_opc(uint64_t w0) { return (uint32_t)(w0 >> 8) & 255u; }
// an Input record of either domain (a record lk_malformed passes)
LK_HD inline bool lk_is_input(uint64_t w0) { return ((uint32_t)w0 & 0xFFFEu) == 0; }

// the malformed-record rule (rv_program_to_bincode's): RV_E_BAD_OP or 0
LK_HD inline int lk_malformed(uint64_t w0) {
    const uint32_t dom = lk_dom(w0);
    if ((w0 >> 16) & 0xFFFFu) return RV_E_BAD_OP;
    if (dom > RV_DOM_SIZEHINT) return RV_E_BAD_OP;
    if (dom <= RV_DOM_Z64 && lk_opc(w0) > RV_OP_CONST) return RV_E_BAD_OP;
    return 0;
}

// THE FIELD TABLE: which fields of a GF(2) or Z64 record name a wire of the record's domain.  (B2A: dst names a Z64 wire and a the
// lowest of 64 GF(2) wires; a SizeHint names none.)
enum { LK_DST = 1, LK_A = 2, LK_B = 4 };
LK_HD inline uint32_t lk_fields(uint32_t opc) {
    uint32_t f = 0;
    if (opc != RV_OP_ASSERTZERO) f |= LK_DST;
    if (opc != RV_OP_INPUT && opc != RV_OP_RANDOM && opc != RV_OP_CONST) f |= LK_A;
    if (opc == RV_OP_ADD || opc == RV_OP_SUB || opc == RV_OP_MUL) f |= LK_B;
    return f;
}

// THE JUDGE of a block record against the block's stated counts: RV_E_BAD_OP, RV_E_UNSUPPORTED (a SizeHint), RV_E_WIRE_OOB or 0
LK_HD inline int lk_judge(const uint64_t w[3], uint64_t z64_wires, uint64_t gf2_wires) {
    if (const int c = lk_malformed(w[0])) return c;
    const uint32_t dom = lk_dom(w[0]);
    if (dom == RV_DOM_SIZEHINT) return RV_E_UNSUPPORTED;
    const uint64_t dst = w[0] >> 32, a = w[1] & 0xFFFFFFFFull, b = w[1] >> 32;
    if (dom == RV_DOM_B2A) return (dst >= z64_wires || a + 64 > gf2_wires) ? RV_E_WIRE_OOB : 0;
    const uint64_t n = dom == RV_DOM_GF2 ? gf2_wires : z64_wires;
    const uint32_t f = lk_fields(lk_opc(w[0]));
    if (((f & LK_DST) && dst >= n) || ((f & LK_A) && a >= n) || ((f & LK_B) && b >= n)) return RV_E_WIRE_OOB;
    return 0;
}

// what a record of head or tail asks of the wire counts (the largest-index rule of reverie_amd.ops.largest_wires); the record has
// passed lk_malformed
LK_HD inline void lk_need(const uint64_t w[3], uint64_t& z64, uint64_t& gf2) {
    const uint32_t dom = lk_dom(w[0]);
    const uint64_t dst = w[0] >> 32, a = w[1] & 0xFFFFFFFFull, b = w[1] >> 32;
    z64 = gf2 = 0;
    if (dom == RV_DOM_SIZEHINT) {
        z64 = a, gf2 = b;
    } else if (dom == RV_DOM_B2A) {
        z64 = dst + 1, gf2 = a + 64;
    } else {
        const uint32_t f = lk_fields(lk_opc(w[0]));
        uint64_t hi = 0;
        if (f & LK_DST) hi = dst + 1;
        if ((f & LK_A) && a + 1 > hi) hi = a + 1;
        if ((f & LK_B) && b + 1 > hi) hi = b + 1;
        (dom == RV_DOM_GF2 ? gf2 : z64) = hi;
    }
}

// THE REWRITE: the record an instance whose wires start at (zb, gb) emits for block record w (one that lk_judge passes).  binding
// is looked at for an Input alone: the entry of its port.
LK_HD inline void lk_rewrite(const uint64_t w[3], uint32_t zb, uint32_t gb, uint32_t binding, uint64_t o[3]) {
    const uint32_t dom = lk_dom(w[0]);
    uint32_t dst = (uint32_t)(w[0] >> 32), a = (uint32_t)w[1], b = (uint32_t)(w[1] >> 32);
    if (dom == RV_DOM_B2A) {
        dst += zb, a += gb;
    } else if (dom <= RV_DOM_Z64) {
        const uint32_t base = dom == RV_DOM_GF2 ? gb : zb;
        const uint32_t f = lk_fields(lk_opc(w[0]));
        if (f & LK_DST) dst += base;
        if (f & LK_A) a += base;
        if (f & LK_B) b += base;
    }
    // (one exit, the two forms chosen field by field: the kernel's lanes stay together)
    const bool copy = lk_is_input(w[0]) && binding != RV_LINK_WITNESS;  // a copy of the wire the port is bound to
    o[0] = (copy ? (uint64_t)dom | (uint64_t)RV_OP_ADDCONST << 8 : w[0] & 0xFFFFFFFFull) | (uint64_t)dst << 32;
    o[1] = copy ? (uint64_t)binding : (uint64_t)a | (uint64_t)b << 32;
    o[2] = copy ? 0 : w[2];
}

// ---- the searches of the kernels: `off` is a nondecreasing array (a pointer, or anything else that takes an index) ----
// the last index in [lo, hi) whose entry is <= k; off[lo] <= k is the caller's word
template <class Off>
LK_HD inline uint64_t lk_last_le(const Off& off, uint64_t lo, uint64_t hi, uint64_t k) {
    while (hi - lo > 1) {
        const uint64_t mid = lo + (hi - lo) / 2;
        if ((uint64_t)off[mid] <= k) lo = mid;
        else hi = mid;
    }
    return lo;
}
// the same from a start that is near the answer: doubling steps from lo, then lk_last_le between the last two probes
template <class Off>
LK_HD inline uint64_t lk_gallop(const Off& off, uint64_t lo, uint64_t hi, uint64_t k) {
    uint64_t step = 1, top = lo + 1 < hi ? lo + 1 : hi;
    while (top < hi && (uint64_t)off[top] <= k) {
        lo = top, step <<= 1;
        top = hi - lo > step ? lo + step : hi;
    }
    return lk_last_le(off, lo, top, k);
}

// ---- a tile's image: its bytes lie in LDS at the position modulo 16 they have in d_ops (sh = 0 or 8: d_ops is 8-byte aligned), so
// the image is [sh, span) of 16-byte chunks that are aligned in d_ops too.  Chunk c (a multiple of 16): 3 = one 16-byte store,
// 1 / 2 = the 8-byte piece at c / at c + 8 alone (the image's two ends), 0 = nothing. ----
LK_HD inline uint32_t lk_chunk(uint32_t c, uint32_t sh, uint32_t span) {
    return (c >= sh && c + 8 <= span ? 1u : 0u) | (c + 8 >= sh && c + 16 <= span ? 2u : 0u);
}
constexpr uint32_t LK_IMAGE = 8 + LINK_TILE * 24 + 8;  // the shift, the records, the last chunk's other half

// where the lists of a descriptor lie in the plan's one array of records, and the totals the emit kernel goes by
struct LkBlock {
    uint64_t off, n_ops;  // the block's records: [off, off + n_ops) of the array
    uint64_t z64_wires, gf2_wires;
};

// ---- the host's share of the decisions (plain C++: rv_link and rv_link_plan_create both call these) ----
// decision (1) on everything but the device pointers -> RV_OK, RV_E_ARG or RV_E_UNSUPPORTED; *block_ops = the blocks' records in all
inline int lk_check_args(const rv_link_desc* d, uint64_t* block_ops) {
    if (!d) return RV_E_ARG;
    if ((d->n_blocks && !d->blocks) || (d->n_instances && !d->block_of) || (d->n_bindings && !d->bindings) || (d->n_head && !d->head) ||
        (d->n_tail && !d->tail))
        return RV_E_ARG;
    uint64_t total = 0;
    bool many = false;
    for (uint64_t b = 0; b < d->n_blocks; b++) {
        const rv_link_block& k = d->blocks[b];
        if ((k.n_ops && !k.ops) || k.z64_wires > (1ull << 32) || k.gf2_wires > (1ull << 32)) return RV_E_ARG;
        if (k.n_ops >= LK_MAX_BLOCK_OPS - total) many = true;
        else total += k.n_ops;
    }
    if (many || d->n_instances >= LK_MAX_INSTANCES) return RV_E_UNSUPPORTED;
    *block_ops = total;
    return RV_OK;
}
// decisions (3) and (4) for one of the two host lists, with its needs and its Input counts
struct LkEnds {
    uint64_t z64 = 0, gf2 = 0, in_gf2 = 0, in_z64 = 0;
};
inline int lk_judge_end(const rv_op* ops, uint64_t n, LkEnds& e) {
    const uint64_t* w = reinterpret_cast<const uint64_t*>(ops);
    for (uint64_t i = 0; i < n; i++, w += 3) {
        if (const int c = lk_malformed(w[0])) return c;
        uint64_t z, g;
        lk_need(w, z, g);
        if (z > e.z64) e.z64 = z;
        if (g > e.gf2) e.gf2 = g;
        if (lk_is_input(w[0])) (lk_dom(w[0]) == RV_DOM_GF2 ? e.in_gf2 : e.in_z64)++;
    }
    return RV_OK;
}
// the tail of decision (5): the result's wire counts from the ends' needs and the instances' sums -> RV_OK or RV_E_UNSUPPORTED
inline int lk_wire_counts(const rv_link_desc* d, const LkEnds& e, uint64_t z_sum, uint64_t g_sum, uint64_t* z64_wires, uint64_t* gf2_wires) {
    uint64_t z = e.z64, g = e.gf2;
    if (d->n_instances) {
        // (z_sum, g_sum < 2^63: below 2^31 instances of at most 2^32 wires each)
        if (d->z64_base > 0xFFFFFFFFull || d->gf2_base > 0xFFFFFFFFull || d->z64_base + z_sum > 0xFFFFFFFFull || d->gf2_base + g_sum > 0xFFFFFFFFull)
            return RV_E_UNSUPPORTED;
        if (d->z64_base + z_sum > z) z = d->z64_base + z_sum;
        if (d->gf2_base + g_sum > g) g = d->gf2_base + g_sum;
    }
    if (z > (1ull << 32) || g > (1ull << 32)) return RV_E_UNSUPPORTED;
    *z64_wires = z, *gf2_wires = g;
    return RV_OK;
}

}  // namespace rv

#if defined(__HIPCC__)
#include "compile_dev.h"

namespace rv {

struct LinkPlan;
// The plan of a descriptor that passed lk_check_args (block_ops: its total), whose device pointers (flags) the caller has checked.
// *code = rv_link's code for the descriptor; a plan is made (and *info filled) only for RV_OK.  Runs on st and waits for it; the
// plan's arrays come from A and stay until link_plan_destroy.  RV_OK (code, plan and info filled), RV_E_NOMEM or RV_E_DEVICE.
int link_plan_create(hipStream_t st, const DevAlloc& A, const rv_link_desc* d, uint64_t block_ops, uint32_t flags, int* code, LinkPlan** plan,
                     rv_link_info* info);
const rv_link_info& link_plan_info(const LinkPlan* p);
// records [first, first + n) (inside the list, n < LK_MAX_EMIT) into d_ops; one synchronisation of the stream, at the end.
// RV_OK (piece filled), RV_E_NOMEM or RV_E_DEVICE.
int link_plan_emit(LinkPlan* p, uint64_t first, uint64_t n, rv_op* d_ops, rv_link_piece* piece);
void link_plan_destroy(LinkPlan* p);

}  // namespace rv
#endif
