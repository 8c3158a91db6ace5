// Bristol / Bristol Fashion gate lines parsed on the GPU (bristol_dev.hip): rv_bristol_parse's records, byte for byte, and its return
// code, for a text that lies in device memory -- whole (rv_bristol_parse_device) or in windows (rv_bristol_reader_*).  The rule is in
// include/reverie_amd.h, the stages in DESIGN §18 and at the head of bristol_dev.hip.  The header lines are parsed on the host
// (bristol.cpp: one implementation for all parsers).
//
// Everything up to the `rv` device entry points at the end is plain C++ (no HIP header is needed: the CPU model of
// tests/bristol_window_model.cpp compiles it with g++): what one lane of a tile does, what one line needs (the token cursor, the
// validation, the emission), and the state between the windows of a reader.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include <vector>

#include "../../include/reverie_amd.h"

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define BR_HD __host__ __device__
#else
#define BR_HD
#endif

// bristol.cpp: the header lines of text[0, len), a prefix of a text of full_len bytes that reaches the end of the first non-blank gate line
extern "C" int rv_internal_bristol_header(const char* text, size_t len, size_t full_len, int format, int has_expected, size_t n_expected,
                                          rv_bristol_info* info, size_t* gates_offset);

namespace rv {

// bytes of text one workgroup of the tile kernels covers, and gate lines one workgroup of the line kernels covers (the lengths the
// tests go around: rv_hook_bristol_tiles)
constexpr uint32_t BRISTOL_TILE_BYTES = 4096;
constexpr uint32_t BRISTOL_WG_LINES = 256;

// ---- a lane of a tile: 16 bytes as two masks (bit k of lf / tok = byte k is a line feed / a token byte) ----
BR_HD inline void br_class(uint32_t b, int k, uint32_t& lf, uint32_t& tok) {
    if (b == '\n') lf |= 1u << k;
    else if (b != ' ' && b != '\t' && b != '\r') tok |= 1u << k;
}
// the bytes of c[0, 16) that lie in [lo, hi), one at a time (the tile kernels take a lane that lies inside with one 16-byte load)
BR_HD inline void br_classify_bytes(const uint8_t* c, const uint8_t* lo, const uint8_t* hi, uint32_t& lf, uint32_t& tok) {
    lf = tok = 0;
    const int from = c < lo ? (int)(lo - c) : 0, to = hi - c < 16 ? (int)(hi - c) : 16;
    for (int k = from; k < to; k++) br_class(c[k], k, lf, tok);
}
// the lane's scan key: 0 for nothing but whitespace, else (lane + 1) << 1 | "a token follows the lane's last LF"
BR_HD inline uint32_t br_lane_key(uint32_t lane, uint32_t lf, uint32_t tok) {
    const uint32_t after = lf ? tok >> (32 - __builtin_clz(lf)) : tok;
    return (lf | tok) ? ((lane + 1u) << 1 | (after ? 1u : 0u)) : 0u;
}
// bit k: byte k is a gate line's first token byte; s: the lane begins inside a line that already has a token
BR_HD inline uint32_t br_lane_starts(uint32_t lf, uint32_t tok, uint32_t s) {
    uint32_t starts = 0;
    for (int k = 0; k < 16; k++) {
        if ((lf >> k) & 1u) s = 0;
        else if ((tok >> k) & 1u) {
            if (!s) starts |= 1u << k;
            s = 1;
        }
    }
    return starts;
}
// the first lane of a tile that holds anything: does its first count depend on the state the tile begins in?
BR_HD inline uint32_t br_lane_cond(uint32_t lf, uint32_t tok) { return tok && (!lf || __builtin_ffs((int)tok) < __builtin_ffs((int)lf)) ? 1u : 0u; }
// the offset behind the lane's last LF (0: it has none), the lane's first byte at offset `at` of the buffer
BR_HD inline uint32_t br_lane_lf_end(uint32_t lf, uint64_t at) { return lf ? (uint32_t)(at + (32 - __builtin_clz(lf))) : 0u; }
BR_HD inline uint32_t br_tile_key(uint32_t tile, uint32_t last) { return last ? ((tile + 1u) << 1 | (last & 1u)) : 0u; }
BR_HD inline uint32_t br_tile_count(uint32_t meta, uint32_t tin) { return (meta & 0x7FFFFFFFu) - ((meta >> 31) & tin & 1u); }

// ---- which lines of a buffer a call judges ----
// The buffer begins at a line's start and holds `starts` first token bytes; tail_key is the tiles' last scan key (bit 0: a token follows
// the buffer's last LF, so that line is unfinished unless the file ends here: at_end); want = n_gates - lines done before.
struct BrTake {
    uint64_t found;  // final lines in the buffer
    uint64_t take;   // those the call judges and delivers: the first `want` of them
    bool short_file;  // the file ends with fewer lines than the header names: line `found` is the host's RV_E_BAD_OP
    bool last;       // line n_gates - 1 becomes final (or none was due): the assertion pairs go with this call
};
BR_HD inline BrTake br_take(uint64_t starts, uint32_t tail_key, bool at_end, uint64_t want) {
    BrTake t;
    t.found = starts - ((tail_key & 1u) && !at_end ? 1u : 0u);
    t.take = t.found < want ? t.found : want;
    t.short_file = at_end && t.found < want;
    t.last = t.take == want;
    return t;
}
// Lines the line table needs room for.  A line that passes the validation takes 8 bytes with its LF (7 where the file ends without
// one), so more final lines than bytes / 8 + 1 means one of the first bytes / 8 + 2 is bad: lines behind those are never looked at.
BR_HD inline uint64_t br_line_cap(uint64_t bytes, uint64_t want) {
    const uint64_t cap = bytes / 8 + 2;
    return cap < want ? cap : want;
}

// ---- one line ----
// a cursor over one line's tokens
struct BrCur {
    const uint8_t* p;
    const uint8_t* hi;
    // the next token, false at the line's end.  v: its value by the host's rule (to_u64 of bristol.cpp); st: 0 for a number below 2^32,
    // RV_E_BAD_OP when not all digits, RV_E_UNSUPPORTED when all digits and 2^32 or more; head: its first four bytes, n: its length
    BR_HD bool next(uint64_t& v, int& st, uint32_t& head, uint32_t& n) {
        uint32_t b = 0;
        while (p < hi && ((b = *p) == ' ' || b == '\t' || b == '\r')) p++;
        if (p >= hi || b == '\n') return false;
        v = 0, head = 0, n = 0;
        bool big = false, other = false;
        do {
            if (n < 4) head |= b << (8 * n);
            n++;
            if (b < '0' || b > '9') other = true;
            else if (!big && !other) {
                v = v * 10 + (b - '0');
                big = v > 0xFFFFFFFFull;
            }
            p++;
        } while (p < hi && (b = *p) != ' ' && b != '\t' && b != '\r' && b != '\n');
        st = other ? RV_E_BAD_OP : big ? RV_E_UNSUPPORTED : 0;
        return true;
    }
    BR_HD bool next(uint64_t& v) {
        int st;
        uint32_t head, n;
        return next(v, st, head, n);
    }
};
constexpr uint32_t br_kind3(char a, char b, char c) { return (uint32_t)a | (uint32_t)b << 8 | (uint32_t)c << 16; }
enum { BR_NONE, BR_XOR, BR_AND, BR_INV, BR_EQW, BR_EQ, BR_MAND };
BR_HD inline int br_kind_of(uint32_t head, uint32_t n) {  // (case-sensitive, as the host's string compares)
    if (n == 3) {
        if (head == br_kind3('X', 'O', 'R')) return BR_XOR;
        if (head == br_kind3('A', 'N', 'D')) return BR_AND;
        if (head == br_kind3('I', 'N', 'V') || head == br_kind3('N', 'O', 'T')) return BR_INV;
        if (head == br_kind3('E', 'Q', 'W')) return BR_EQW;
    }
    if (n == 2 && head == ((uint32_t)'E' | (uint32_t)'Q' << 8)) return BR_EQ;
    if (n == 4 && head == (br_kind3('M', 'A', 'N') | (uint32_t)'D' << 24)) return BR_MAND;
    return BR_NONE;
}

// The line whose first token byte is p: its code by the host's order of decisions, its record count (1; nout for MAND) and its class
// (0 and, 1 xor, 2 inv, 3 other; -1: none).  One walk with constant state, so a MAND line of any length costs O(tokens).
struct BrLine {
    int code, cl;
    uint64_t recs;
};
BR_HD inline BrLine br_validate(const uint8_t* p, const uint8_t* hi, uint64_t n_wires) {
    BrLine r{0, -1, 0};
    BrCur c{p, hi};
    // every token but the last is a number; which one is the last is known when the walk ends, so a token waits one step
    uint64_t v = 0, pv = 0, nin = 0, nout = 0, v2 = 0, v3 = 0, ntok = 0;
    int st = 0, pst = 0, numerr = 0;
    uint32_t head = 0, n = 0;
    bool oob = false;  // a number from the third on is no wire
    while (c.next(v, st, head, n)) {
        if (ntok) {
            const uint64_t k = ntok - 1;
            if (!numerr) {
                if (pst) numerr = pst;
                else if (k == 0) nin = pv;
                else if (k == 1) nout = pv;
                else {
                    if (k == 2) v2 = pv;
                    if (k == 3) v3 = pv;
                    oob |= pv >= n_wires;
                }
            }
        }
        pv = v, pst = st, ntok++;
        if (numerr && ntok >= 4) break;
    }
    const int kind = br_kind_of(head, n);
    if (ntok < 4) r.code = RV_E_BAD_OP;
    else if (numerr) r.code = numerr;
    else if (ntok - 1 != 2 + nin + nout) r.code = RV_E_BAD_OP;
    else if (kind == BR_XOR || kind == BR_AND) {
        if (nin != 2 || nout != 1) r.code = RV_E_BAD_OP;
        else if (oob) r.code = RV_E_WIRE_OOB;
        r.cl = kind == BR_AND ? 0 : 1, r.recs = 1;
    } else if (kind == BR_INV || kind == BR_EQW) {
        if (nin != 1 || nout != 1) r.code = RV_E_BAD_OP;
        else if (oob) r.code = RV_E_WIRE_OOB;
        r.cl = kind == BR_INV ? 2 : 3, r.recs = 1;
    } else if (kind == BR_EQ) {  // the "input" is the literal
        if (nin != 1 || nout != 1 || v2 > 1) r.code = RV_E_BAD_OP;
        else if (v3 >= n_wires) r.code = RV_E_WIRE_OOB;
        r.cl = 3, r.recs = 1;
    } else if (kind == BR_MAND) {
        if (nin != 2 * nout || nout == 0) r.code = RV_E_BAD_OP;
        else if (oob) r.code = RV_E_WIRE_OOB;
        r.cl = 0, r.recs = nout;
    } else {
        r.code = RV_E_BAD_OP;
    }
    if (r.code) r.recs = 0, r.cl = -1;
    return r;
}

// record `at` of out: three 8-byte stores, no byte left unwritten
BR_HD inline void br_put(uint64_t* out, uint64_t at, uint32_t opcode, uint32_t dst, uint32_t a, uint32_t b, uint64_t imm) {
    uint64_t* r = out + at * 3;  // rv_op: domain (GF(2): 0), opcode, reserved, dst | a, b | imm
    r[0] = (uint64_t)opcode << 8 | (uint64_t)dst << 32;
    r[1] = (uint64_t)a | (uint64_t)b << 32;
    r[2] = imm;
}
// the records of a line that passed br_validate, from record `at` on; a MAND line of more than one lane with three cursors in step
// (in[k], in[nout + k], out[k])
BR_HD inline void br_emit(const uint8_t* p, const uint8_t* hi, uint64_t* out, uint64_t at) {
    const BrCur start{p, hi};
    BrCur c = start;
    uint64_t v = 0, w[5] = {0, 0, 0, 0, 0}, ntok = 0;
    int st;
    uint32_t head = 0, n = 0;
    while (c.next(v, st, head, n)) {
        if (ntok < 5) w[ntok] = v;
        ntok++;
    }
    switch (br_kind_of(head, n)) {
    case BR_XOR: br_put(out, at, RV_OP_ADD, (uint32_t)w[4], (uint32_t)w[2], (uint32_t)w[3], 0); break;
    case BR_AND: br_put(out, at, RV_OP_MUL, (uint32_t)w[4], (uint32_t)w[2], (uint32_t)w[3], 0); break;
    case BR_INV: br_put(out, at, RV_OP_ADDCONST, (uint32_t)w[3], (uint32_t)w[2], 0, 1); break;
    case BR_EQW: br_put(out, at, RV_OP_ADDCONST, (uint32_t)w[3], (uint32_t)w[2], 0, 0); break;
    case BR_EQ: br_put(out, at, RV_OP_CONST, (uint32_t)w[3], 0, 0, w[2]); break;
    case BR_MAND: {
        const uint64_t nout = w[1];
        BrCur ca = start, cb, co;
        ca.next(v), ca.next(v);
        cb = ca;
        for (uint64_t k = 0; k < nout; k++) cb.next(v);
        co = cb;
        for (uint64_t k = 0; k < nout; k++) co.next(v);
        for (uint64_t k = 0; k < nout; k++) {
            uint64_t a = 0, b = 0, o = 0;
            ca.next(a), cb.next(b), co.next(o);
            br_put(out, at + k, RV_OP_MUL, (uint32_t)o, (uint32_t)a, (uint32_t)b, 0);
        }
        break;
    }
    default: break;
    }
}
BR_HD inline void br_emit_input(uint64_t* out, uint64_t at, uint64_t w) { br_put(out, at, RV_OP_INPUT, (uint32_t)w, 0, 0, 0); }
// AddConst(tmp, w, expected) + AssertZero(tmp) for output k of n_pairs (the last n_pairs wires)
BR_HD inline void br_emit_pair(uint64_t* out, uint64_t at, uint64_t n_wires, uint64_t n_pairs, uint64_t k, uint32_t bit) {
    const uint32_t tmp = (uint32_t)(n_wires + k);
    br_put(out, at, RV_OP_ADDCONST, tmp, (uint32_t)(n_wires - n_pairs + k), 0, bit & 1u);
    br_put(out, at + 1, RV_OP_ASSERTZERO, 0, tmp, 0, 0);
}

// ---- a text read in windows: the state between the feeds (rv_bristol_reader_*; host code) ----
// A feed's buffer is the carry (the bytes behind the last LF fed so far: the unfinished line), then -- in the feed that completes the
// header -- the header bytes kept on the host that lie behind the last header line, then the feed's own bytes.
struct BrWindowState {
    uint64_t file_len = 0, fed = 0;
    int format = 0;
    bool has_expected = false;
    size_t n_expected = 0;
    int code = 0;  // the text's code: the reader takes nothing more
    // the header: the first bytes of the file, until they hold four whole non-blank lines or the file ends
    bool have_header = false;
    std::vector<char> head;
    size_t head_seen = 0;
    int head_lines = 0;
    bool head_token = false;
    size_t gates_offset = 0;
    rv_bristol_info info = {};  // the header's counts; the class counters of the lines delivered so far
    uint64_t n_pairs = 0;
    // the gate lines
    uint64_t lines_done = 0, ops_done = 0;
    bool inputs_out = false, pairs_out = false;
    uint64_t carry = 0;  // bytes of the unfinished line kept in device memory
};
inline void br_window_begin(BrWindowState& s, uint64_t file_len, int format, bool has_expected, size_t n_expected) {
    s = BrWindowState{};
    s.file_len = file_len, s.format = format, s.has_expected = has_expected, s.n_expected = n_expected;
}
inline bool br_window_complete(const BrWindowState& s) { return s.have_header && s.lines_done == s.info.n_gates && s.pairs_out; }
// Header bytes wanted next from a feed of which `left` bytes are not yet taken (0: none, the header code can run or the feed is used
// up): 4096 at first, then as many as are held, as bristol_device_prefix takes them.
inline size_t br_window_head_need(const BrWindowState& s, size_t left) {
    if (s.have_header || s.head_lines >= 4) return 0;
    const size_t want = s.head.size() < 4096 ? 4096 - s.head.size() : s.head.size();
    return left < want ? left : want;
}
// the bytes just appended to s.head are looked at: true when the header code can run (fed_after: bytes of the file fed with them)
inline bool br_window_head_scan(BrWindowState& s, uint64_t fed_after) {
    for (; s.head_seen < s.head.size() && s.head_lines < 4; s.head_seen++) {
        const char c = s.head[s.head_seen];
        if (c == '\n') s.head_lines += s.head_token, s.head_token = false;
        else if (c != ' ' && c != '\t' && c != '\r') s.head_token = true;
    }
    return s.head_lines >= 4 || fed_after == s.file_len;
}
// the shared header code on the bytes held; its code is the feed's
inline int br_window_header(BrWindowState& s) {
    rv_bristol_info bi;
    size_t off = 0;
    const int rc = rv_internal_bristol_header(s.head.empty() ? "" : s.head.data(), s.head.size(), (size_t)s.file_len, s.format, s.has_expected ? 1 : 0,
                                              s.n_expected, &bi, &off);
    if (rc) return s.code = rc;
    s.info = bi;
    s.n_pairs = s.has_expected ? bi.n_outputs : 0;
    s.info.gf2_wires = bi.n_wires + s.n_pairs;
    s.gates_offset = off;
    s.have_header = true;
    return RV_OK;
}
// what one feed's kernels are given
struct BrWindowLaunch {
    uint64_t want;      // gate lines still due
    uint64_t n_inputs;  // Input records that lead this feed's piece
    uint64_t n_pairs;   // assertion pairs that end the piece of the feed that makes the last line final (0: none, or they are out)
    bool at_end;        // the buffer's last byte is the file's
};
inline BrWindowLaunch br_window_launch(const BrWindowState& s, uint64_t len) {
    return BrWindowLaunch{s.info.n_gates - s.lines_done, s.inputs_out ? 0 : s.info.n_inputs, s.pairs_out ? 0 : s.n_pairs, s.fed + len == s.file_len};
}
// and what they answer (the words of one call, fetched)
struct BrWindowResult {
    int code = 0;             // the first bad line's code among the lines judged (the short file's among them)
    uint64_t n_lines = 0;     // lines judged and delivered
    bool last = false;        // line n_gates - 1 among them (or none was due)
    uint64_t gate_ops = 0;    // their records
    uint64_t n_and = 0, n_xor = 0, n_inv = 0, n_other = 0;
    uint64_t carry_from = 0;  // the offset behind the buffer's last LF (0: it has none)
};
// the header accumulation of a feed taken back (a feed that fails for a reason other than the text leaves the state as it found it)
struct BrHeadMark {
    size_t size, seen;
    int lines;
    bool token;
};
inline BrHeadMark br_window_mark(const BrWindowState& s) { return BrHeadMark{s.head.size(), s.head_seen, s.head_lines, s.head_token}; }
inline void br_window_rollback(BrWindowState& s, const BrHeadMark& m) {
    s.head.resize(m.size);
    s.head_seen = m.seen, s.head_lines = m.lines, s.head_token = m.token;
    s.have_header = false;
}
// The end of a feed of len bytes whose kernels answered res for a buffer of `bytes` bytes: the code (the text's, too many wires,
// capacity) and the piece; the state moves only with RV_OK.  cap: records d_ops holds (scan: no d_ops).
// the carry a feed leaves: what lies behind its buffer's last LF, unless nothing more is judged
inline uint64_t br_window_carry(const BrWindowLaunch& l, const BrWindowResult& res, uint64_t bytes) {
    return res.last || l.at_end ? 0 : bytes - res.carry_from;
}
inline int br_window_done(BrWindowState& s, uint64_t len, uint64_t bytes, const BrWindowLaunch& l, const BrWindowResult& res, bool scan, uint64_t cap,
                          rv_bristol_piece* piece) {
    *piece = rv_bristol_piece{};
    if (res.code) return s.code = res.code;
    if (res.last && s.info.gf2_wires > 0xFFFFFFFFull) return s.code = RV_E_UNSUPPORTED;
    const uint64_t pairs = res.last ? l.n_pairs : 0;
    piece->first_op = s.ops_done, piece->n_ops = l.n_inputs + res.gate_ops + 2 * pairs;
    piece->n_input_gf2 = l.n_inputs;
    piece->first_line = s.lines_done, piece->n_lines = res.n_lines;
    if (!scan && cap < piece->n_ops) return RV_E_ARG;  // (the same bytes are fed again)
    s.fed += len;
    s.inputs_out = true;
    s.lines_done += res.n_lines, s.ops_done += piece->n_ops;
    s.info.n_and += res.n_and, s.info.n_xor += res.n_xor, s.info.n_inv += res.n_inv, s.info.n_other += res.n_other;
    if (res.last) s.pairs_out = true;
    s.carry = br_window_carry(l, res, bytes);
    return RV_OK;
}
// a feed that launches nothing: header bytes alone, or bytes behind the last gate line
inline void br_window_skip(BrWindowState& s, uint64_t len, rv_bristol_piece* piece) {
    *piece = rv_bristol_piece{};
    piece->first_op = s.ops_done, piece->first_line = s.lines_done;
    s.fed += len;
}
inline int br_window_finish(const BrWindowState& s, rv_bristol_info* info) {
    if (s.code || !br_window_complete(s)) return RV_E_ARG;
    if (info) *info = s.info;
    return RV_OK;
}

}  // namespace rv

#if defined(__HIPCC__)
#include "compile_dev.h"

namespace rv {

struct BristolGates {
    int code = 0;          // RV_OK or the first bad gate line's code
    uint64_t gate_ops = 0;  // records the gate lines stand for (with RV_OK)
    uint64_t n_and = 0, n_xor = 0, n_inv = 0, n_other = 0;
    bool written = false;  // the records were written (the capacity sufficed)
};

// d_text[0, len): the whole text in device memory (len < 2^32), its gate lines from gates_offset on; n_gates, n_wires, n_inputs from the
// header.  d_ops / cap_ops: where the records go (null: nowhere); the assertion pairs of d_expected (device memory, n_pairs bytes, one
// per output wire; n_pairs 0: none) follow the gates.  Records are written only when there is no error and
// n_inputs + gate ops + 2 * pairs <= cap_ops -- decided on the device, so the stream is synchronised once, at the end.  Work memory
// from A, given back before the call returns.  RV_OK (res filled), RV_E_NOMEM or RV_E_DEVICE.
int bristol_gates_device(hipStream_t st, const DevAlloc& A, const uint8_t* d_text, size_t len, size_t gates_offset, uint64_t n_gates, uint64_t n_wires,
                         uint64_t n_inputs, const uint8_t* d_expected, uint64_t n_pairs, rv_op* d_ops, uint64_t cap_ops, BristolGates* res);

// One feed of a reader: d_buf[0, bytes) is the feed's buffer (16-byte aligned, bytes < 2^32; it begins at a line's start).  The lines
// that are final (BrTake) are judged and, where d_ops is given, nothing is wrong and n_inputs + gate ops + 2 * pairs <= cap_ops,
// written: the inputs first, the pairs (when the last line is among them) last.  Synchronises the stream once.
int bristol_window_device(hipStream_t st, const DevAlloc& A, const uint8_t* d_buf, size_t bytes, const BrWindowLaunch& l, uint64_t n_wires,
                          const uint8_t* d_expected, rv_op* d_ops, uint64_t cap_ops, BrWindowResult* res);

}  // namespace rv
#endif
