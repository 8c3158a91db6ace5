// Constants folded in op lists: on the host (rv_ops_fold, fold.cpp) and on the GPU (fold_dev.hip).  The rule is in
// include/reverie_amd.h, the steps in DESIGN §24 and at the head of fold_dev.hip.
//
// ONE RECORD'S PART IN THE RULE -- whether it is known before anything is propagated (fd_seed), whether it is known given what is
// known of its reads (fd_known), the value of a known record (fd_eval, fd_b2a_bit), the record that replaces it (fd_rewrite) and the
// class it is counted in (fd_class) -- is decided here and nowhere else.  What a record defines and reads, compile_ops' check of it,
// the search that resolves a read and the way a tile's image is cut into stores are prune.h's.  The host sweep, the kernels and the
// CPU model of tests/fold_model.cpp all call these functions.
//
// Everything here is plain C++ (the CPU model compiles it with g++); fold_dev.h holds what needs HIP.
#pragma once
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
// Is it known before any propagation?  unwritten[k]: read k names an index no earlier op wrote (the zero wire, known 0)
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

}  // namespace rv
