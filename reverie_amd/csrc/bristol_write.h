// Bristol Fashion text written from rv_op records: on the host (rv_bristol_write, bristol.cpp), on the GPU (bristol_write.hip) and in
// windows (rv_bristol_writer_*).  The rule is in include/reverie_amd.h, the stages in DESIGN §20 and at the head of bristol_write.hip.
//
// ONE RECORD'S LINE -- its code, its length and its bytes -- is decided here and nowhere else (bw_judge, bw_emit), and so are the
// header lines (bw_header): the host writer, the kernels and the CPU model of tests/bristol_write_asan.cpp all call these functions.
//
// Everything up to the `rv` functions at the end is plain C++ (no HIP header is needed: the CPU model compiles it with g++).
#pragma once
#include <stdint.h>

#include "../../include/reverie_amd.h"

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define BW_HD __host__ __device__
#else
#define BW_HD
#endif

namespace rv {

// records per workgroup of the lengths and emit kernels (rv_hook_bristol_write_tiles reports it)
constexpr uint32_t BRISTOL_WRITE_TILE = 256;
// records per workgroup of the scan over the line lengths
constexpr uint32_t BRISTOL_WRITE_SCAN_BLOCK = 2048;
// "2 1 " + three numbers of ten digits with a blank behind each + "XOR\n"
constexpr uint32_t BW_MAX_LINE = 41;
// "%d %d\n1 %d\n1 %d\n\n" of four 64-bit numbers (20 digits each) is 89 bytes
constexpr uint32_t BW_MAX_HEADER = 96;
constexpr uint64_t BW_NO_ERR = ~0ull;

// decimal digits of v, by comparisons
BW_HD inline uint32_t bw_digits(uint32_t v) {
    return 1u + (v >= 10u) + (v >= 100u) + (v >= 1000u) + (v >= 10000u) + (v >= 100000u) + (v >= 1000000u) + (v >= 10000000u) + (v >= 100000000u) +
           (v >= 1000000000u);
}
BW_HD inline uint32_t bw_digits64(uint64_t v) {
    uint32_t n = 1;
    for (uint64_t p = 10; n < 20 && v >= p; p *= 10) n++;  // (10^19 < 2^64 <= 10^20: p never wraps before n reaches 20)
    return n;
}
BW_HD inline uint32_t bw_div10(uint32_t v) { return (uint32_t)(((uint64_t)v * 0xCCCCCCCDull) >> 35); }  // v / 10 for every 32-bit v

// The record at list position `pos` as three 64-bit words (domain | opcode << 8 | reserved << 16 | dst << 32, a | b << 32, imm).
// in_run: the position lies in the leading run of GF(2) Input records (whole list: the record is an Input and so is every record
// before it; in windows: pos < n_inputs).  n_wires: the stated wire count, 0: none is stated.
// -> the record's code, decided in the order of include/reverie_amd.h: RV_E_BAD_OP (reserved != 0, an unknown domain or opcode --
// rv_program_to_bincode's rule: the opcode byte of a B2A or SizeHint record is not looked at), RV_E_UNSUPPORTED (what Bristol text
// cannot say), RV_E_WIRE_OOB (an index the line names at or above a stated n_wires), or 0.  len: the bytes of its line (0: an Input
// record, or a record with a code).  need: the largest index the record names, plus one (0 with a code).
BW_HD inline int bw_judge(const uint64_t w[3], uint64_t pos, bool in_run, uint64_t n_wires, uint32_t& len, uint64_t& need) {
    len = 0, need = 0;
    const uint32_t dom = (uint32_t)w[0] & 255u, opc = (uint32_t)(w[0] >> 8) & 255u;
    if ((w[0] >> 16) & 0xFFFFu) return RV_E_BAD_OP;
    if (dom > RV_DOM_SIZEHINT) return RV_E_BAD_OP;
    if (dom <= RV_DOM_Z64 && opc > RV_OP_CONST) return RV_E_BAD_OP;
    if (dom != RV_DOM_GF2) return RV_E_UNSUPPORTED;
    const uint32_t dst = (uint32_t)(w[0] >> 32), a = (uint32_t)w[1], b = (uint32_t)(w[1] >> 32);
    if (opc == RV_OP_INPUT) {
        if (!in_run || (uint64_t)dst != pos) return RV_E_UNSUPPORTED;
        need = (uint64_t)dst + 1;  // (no line names it: the header's input count is checked against the wires once, behind the records)
        return 0;
    }
    if (in_run) return RV_E_UNSUPPORTED;  // (in windows: a record below n_inputs that is no Input)
    const bool two = opc == RV_OP_ADD || opc == RV_OP_MUL, one = opc == RV_OP_ADDCONST, cst = opc == RV_OP_CONST;
    if (!(two || one || cst)) return RV_E_UNSUPPORTED;
    if (!two && w[2] > 1) return RV_E_UNSUPPORTED;
    uint32_t hi = dst;
    if (!cst && a > hi) hi = a;
    if (two && b > hi) hi = b;
    if (n_wires && (uint64_t)hi >= n_wires) return RV_E_WIRE_OOB;
    need = (uint64_t)hi + 1;
    len = 4 + bw_digits(cst ? (uint32_t)w[2] : a) + 1 + (two ? bw_digits(b) + 1 : 0) + bw_digits(dst) + 1 + (cst ? 2 : 3) + 1;
    return 0;
}

// v in decimal through put(offset, byte) from offset `at` on -> the offset behind it
template <class Put>
BW_HD inline uint32_t bw_put_u32(uint32_t v, uint32_t at, Put& put) {
    const uint32_t n = bw_digits(v);
    for (uint32_t k = n; k-- > 0;) {
        const uint32_t q = bw_div10(v);
        put(at + k, (uint8_t)('0' + (v - q * 10u)));
        v = q;
    }
    return at + n;
}
template <class Put>
BW_HD inline uint32_t bw_put_u64(uint64_t v, uint32_t at, Put& put) {
    const uint32_t n = bw_digits64(v);
    for (uint32_t k = n; k-- > 0;) {
        put(at + k, (uint8_t)('0' + (uint32_t)(v % 10u)));
        v /= 10u;
    }
    return at + n;
}

// the line of a record bw_judge gave a length (not 0) through put(offset, byte): exactly that many bytes
template <class Put>
BW_HD inline void bw_emit(const uint64_t w[3], Put put) {
    const uint32_t opc = (uint32_t)(w[0] >> 8) & 255u;
    const uint32_t dst = (uint32_t)(w[0] >> 32), a = (uint32_t)w[1], b = (uint32_t)(w[1] >> 32);
    const bool two = opc == RV_OP_ADD || opc == RV_OP_MUL, cst = opc == RV_OP_CONST;
    put(0, (uint8_t)(two ? '2' : '1')), put(1, (uint8_t)' '), put(2, (uint8_t)'1'), put(3, (uint8_t)' ');
    uint32_t q = bw_put_u32(cst ? (uint32_t)w[2] : a, 4, put);
    put(q++, (uint8_t)' ');
    if (two) {
        q = bw_put_u32(b, q, put);
        put(q++, (uint8_t)' ');
    }
    q = bw_put_u32(dst, q, put);
    put(q++, (uint8_t)' ');
    // XOR, AND, INV (AddConst 1), EQW (AddConst 0), EQ
#define BW_KIND(c0, c1, c2) ((uint32_t)(c0) | (uint32_t)(c1) << 8 | (uint32_t)(c2) << 16)
    const uint32_t kind = opc == RV_OP_ADD ? BW_KIND('X', 'O', 'R') : opc == RV_OP_MUL ? BW_KIND('A', 'N', 'D') : cst ? BW_KIND('E', 'Q', '\n')
                          : (w[2] & 1u) ? BW_KIND('I', 'N', 'V') : BW_KIND('E', 'Q', 'W');
#undef BW_KIND
    put(q++, (uint8_t)kind), put(q++, (uint8_t)(kind >> 8)), put(q++, (uint8_t)(kind >> 16));
    if (!cst) put(q, (uint8_t)'\n');
}

// "gates wires\n1 inputs\n1 outputs\n\n"
BW_HD inline uint32_t bw_header_len(uint64_t gates, uint64_t wires, uint64_t inputs, uint64_t outputs) {
    return bw_digits64(gates) + 1 + bw_digits64(wires) + 1 + 2 + bw_digits64(inputs) + 1 + 2 + bw_digits64(outputs) + 2;
}
template <class Put>
BW_HD inline uint32_t bw_header(uint64_t gates, uint64_t wires, uint64_t inputs, uint64_t outputs, Put put) {
    uint32_t q = bw_put_u64(gates, 0, put);
    put(q++, (uint8_t)' ');
    q = bw_put_u64(wires, q, put);
    put(q++, (uint8_t)'\n'), put(q++, (uint8_t)'1'), put(q++, (uint8_t)' ');
    q = bw_put_u64(inputs, q, put);
    put(q++, (uint8_t)'\n'), put(q++, (uint8_t)'1'), put(q++, (uint8_t)' ');
    q = bw_put_u64(outputs, q, put);
    put(q++, (uint8_t)'\n'), put(q++, (uint8_t)'\n');
    return q;
}

// What the writers are told, or derive.  whole = 1 (rv_bristol_write_device): first_op 0, the records are the whole list; n_inputs is
// derived (the end of the leading Input run) and so is n_wires where it is 0; the header leads the text.  whole = 0 (one feed of
// rv_bristol_writer_*): the records are list positions first_op .., n_inputs and n_wires (not 0) are the caller's, and the header
// leads the feed's bytes where `header` is set.
struct BwJob {
    uint64_t first_op, total_ops, n_inputs, n_wires, n_outputs;
    uint32_t whole, header;
};
// the checks behind the records (the header checks rv_bristol_parse would make on the text) -> 0 or RV_E_WIRE_OOB
BW_HD inline int bw_header_code(uint64_t wires, uint64_t inputs, uint64_t outputs) { return outputs > wires || inputs > wires ? RV_E_WIRE_OOB : 0; }

}  // namespace rv

#if defined(__HIPCC__)
#include "compile_dev.h"

namespace rv {

struct BristolWrite {
    int code = 0;        // RV_OK, or the code of the first record in list order that has one, or the header checks' RV_E_WIRE_OOB
    bool record = false; // the code is a record's
    uint64_t err_op = 0; // ... at this list position
    uint64_t bytes = 0;  // the bytes of the text, or of the feed (with RV_OK)
    bool written = false;
};
// d_ops[0, n_ops) (n_ops < 2^32) as text at d_text[0, cap) (null: nowhere); written only when no record has a code, the header
// checks pass and bytes <= min(cap, 2^32 - 1) -- decided on the device.  Work memory (4 bytes per record, the scan's sums) from A,
// given back before the call returns; one synchronisation of the stream, at the end.  RV_OK (res filled), RV_E_NOMEM or RV_E_DEVICE.
int bristol_write_device(hipStream_t st, const DevAlloc& A, const rv_op* d_ops, size_t n_ops, const BwJob& job, uint8_t* d_text, uint64_t cap,
                         BristolWrite* res);

}  // namespace rv
#endif
