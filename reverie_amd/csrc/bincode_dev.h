// Program files (bincode 1.3 of Vec<mcircuit::CombineOperation>, program.cpp) read and written on the GPU (bincode_dev.hip):
// rv_program_from_bincode's records and return code for bytes in device memory, rv_program_to_bincode's bytes for records there.
// The rule is in include/reverie_amd.h, the stages in DESIGN §19 and at the head of bincode_dev.hip.
//
// THE LAYOUT TABLE (BC_LAYOUT) is the one place that knows the file's records: which tags lead a record and which of dst / a / b /
// imm follow, in that order, the immediate one byte (bool) or eight (u64).  Record lengths, the walk, the decode, the writer and the
// CPU model of tests/bincode_walk_asan.cpp are all derived from it; the variant order is the one SURVEY A.7 recalls, and correcting it
// is an edit of this table (and of program.cpp, which stays the definition).
//
// Everything up to the `rv` functions at the end is plain C++ (no HIP header is needed: the CPU model compiles it with g++).
#pragma once
#include <stdint.h>

#include "../../include/reverie_amd.h"

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define BC_HD __host__ __device__
#else
#define BC_HD
#endif

namespace rv {

// bytes of the file one workgroup of the walk and decode kernels covers (tiles are counted from data[0], whatever its address), and
// tiles one workgroup of the composing scan covers (the lengths the tests go around: rv_hook_bincode_tiles)
constexpr uint32_t BINCODE_TILE_BYTES = 4096;
constexpr uint32_t BINCODE_SCAN_TILES = 256;

// ---- the layout table ----
enum : uint8_t { BC_DST = 1, BC_A = 2, BC_B = 4, BC_IMM1 = 8, BC_IMM8 = 16 };
struct BcLayout {
    uint8_t head;    // tag bytes: 8 = u32 domain + u32 opcode, 4 = u32 domain alone, 0 = no such record
    uint8_t fields;  // BC_* of the fields that follow, in the order dst, a, b (u64 each), imm
};
constexpr uint32_t BC_DOMAINS = 4, BC_OPCODES = 10;
#define BC_OPERATION(IMM)                                                                                                                        \
    {                                                                                                                                            \
        {8, BC_DST}, {8, BC_DST}, {8, BC_DST | BC_A | BC_B}, {8, BC_DST | BC_A | IMM}, {8, BC_DST | BC_A | BC_B}, {8, BC_DST | BC_A | IMM},       \
            {8, BC_DST | BC_A | BC_B}, {8, BC_DST | BC_A | IMM}, {8, BC_A}, {8, BC_DST | IMM}                                                      \
    }
constexpr BcLayout BC_LAYOUT[BC_DOMAINS][BC_OPCODES] = {
    BC_OPERATION(BC_IMM1),  // RV_DOM_GF2: Operation<bool>, opcodes RV_OP_INPUT .. RV_OP_CONST
    BC_OPERATION(BC_IMM8),  // RV_DOM_Z64: Operation<u64>
    {{4, BC_DST | BC_A}},   // RV_DOM_B2A(dst, a): no opcode tag, row 0 alone
    {{4, BC_A | BC_B}},     // RV_DOM_SIZEHINT(a, b)
};
#undef BC_OPERATION

constexpr uint32_t bc_row_len(BcLayout r) {
    return r.head ? r.head + 8u * ((r.fields & BC_DST ? 1u : 0u) + (r.fields & BC_A ? 1u : 0u) + (r.fields & BC_B ? 1u : 0u)) + (r.fields & BC_IMM1 ? 1u : 0u) +
                        (r.fields & BC_IMM8 ? 8u : 0u)
                  : 0u;
}
constexpr uint32_t bc_table_len(bool longest) {
    uint32_t v = longest ? 0u : ~0u;
    for (uint32_t d = 0; d < BC_DOMAINS; d++)
        for (uint32_t o = 0; o < BC_OPCODES; o++) {
            const uint32_t l = bc_row_len(BC_LAYOUT[d][o]);
            if (l) v = longest ? (l > v ? l : v) : (l < v ? l : v);
        }
    return v;
}
constexpr uint32_t BC_HEADER_BYTES = 8;                    // the vector's u64 length
constexpr uint32_t BC_MAX_RECORD = bc_table_len(true);     // 32
constexpr uint32_t BC_MIN_RECORD = bc_table_len(false);    // 16
constexpr uint32_t BC_ENTRIES = BC_MAX_RECORD;             // a tile's first record starts at one of this many offsets
constexpr uint32_t BC_TILE_RECORDS = BINCODE_TILE_BYTES / BC_MIN_RECORD;  // records that can start in one tile
static_assert(BC_MAX_RECORD == 32 && BC_MIN_RECORD == 16, "the map entries and the header rule are laid out for records of 16 .. 32 bytes");

// a domain's rows as words the device code shifts instead of loading a table: 6 bits of length, 5 bits of fields per opcode
constexpr uint64_t bc_pack(uint32_t dom, bool lens) {
    uint64_t w = 0;
    for (uint32_t o = 0; o < BC_OPCODES; o++) w |= (uint64_t)(lens ? bc_row_len(BC_LAYOUT[dom][o]) : BC_LAYOUT[dom][o].fields) << ((lens ? 6 : 5) * o);
    return w;
}
constexpr uint64_t BC_LEN0 = bc_pack(0, true), BC_LEN1 = bc_pack(1, true), BC_LEN2 = bc_pack(2, true), BC_LEN3 = bc_pack(3, true);
constexpr uint64_t BC_FLD0 = bc_pack(0, false), BC_FLD1 = bc_pack(1, false), BC_FLD2 = bc_pack(2, false), BC_FLD3 = bc_pack(3, false);
constexpr uint32_t BC_HEADS = BC_LAYOUT[0][0].head | BC_LAYOUT[1][0].head << 4 | BC_LAYOUT[2][0].head << 8 | BC_LAYOUT[3][0].head << 12;

// dom < BC_DOMAINS, opc < BC_OPCODES (0 for a domain without an opcode tag)
BC_HD inline uint32_t bc_head(uint32_t dom) { return (BC_HEADS >> (4 * dom)) & 15u; }
BC_HD inline uint32_t bc_record_len(uint32_t dom, uint32_t opc) {  // 0: no such record
    const uint64_t w = dom == 0 ? BC_LEN0 : dom == 1 ? BC_LEN1 : dom == 2 ? BC_LEN2 : BC_LEN3;
    return (uint32_t)(w >> (6 * opc)) & 63u;
}
BC_HD inline uint32_t bc_fields(uint32_t dom, uint32_t opc) {
    const uint64_t w = dom == 0 ? BC_FLD0 : dom == 1 ? BC_FLD1 : dom == 2 ? BC_FLD2 : BC_FLD3;
    return (uint32_t)(w >> (5 * opc)) & 31u;
}

// ---- the walk ----
// A Reader gives the bytes of one tile: u8 / u32 / u64 at an offset from the tile's first byte (little endian, no alignment).  The
// functions below read only offsets below `avail` -- the tile's bytes and the BC_MAX_RECORD - 1 behind them, clipped to the file's
// length -- so a Reader over exactly those bytes is never asked for another (the CPU model's is a heap block of that size).

// The record that starts at offset p: its length, or 0 where the host parser returns RV_E_BAD_OP for a reason that leaves no length --
// the tags do not lie inside the file, name no record, or the record passes the file's end (program.cpp decides all three the same).
template <class R>
BC_HD inline uint32_t bc_peek(const R& r, uint32_t p, uint32_t avail, uint32_t& dom, uint32_t& opc) {
    if (avail < 4 || p > avail - 4) return 0;
    dom = r.u32(p);
    opc = 0;
    if (dom >= BC_DOMAINS) return 0;
    if (bc_head(dom) == 8) {
        if (avail < 8 || p > avail - 8) return 0;
        opc = r.u32(p + 4);
        if (opc >= BC_OPCODES) return 0;
    }
    const uint32_t len = bc_record_len(dom, opc);
    if (!len || len > avail - p) return 0;
    return len;
}

// One entry of a tile's map: what a walk that enters the tile at offset e < BC_ENTRIES leaves.  Bits 0-5: the offset into the next
// tile at which it leaves (< BC_ENTRIES), or BC_STOP: it met a position bc_peek answers 0 for; bits 6-14: the whole records it
// started in the tile before that.
constexpr uint32_t BC_STOP = 63;
static_assert(BC_TILE_RECORDS < (1u << 9), "a tile's record count takes nine bits of a map entry");
// starts: null, or room for BC_TILE_RECORDS offsets -- where the records begin
// end: null, or where the walk stood when it returned -- the offset it stopped at, or (>= the tile's bytes) the one it left at
template <class R>
BC_HD inline uint32_t bc_walk_tile(const R& r, uint32_t avail, uint32_t entry, uint16_t* starts, uint32_t* end = nullptr) {
    uint32_t p = entry, n = 0, dom, opc;
    while (p < BINCODE_TILE_BYTES) {
        const uint32_t len = bc_peek(r, p, avail, dom, opc);
        if (!len) {
            if (end) *end = p;
            return BC_STOP | n << 6;
        }
        if (starts) starts[n] = (uint16_t)p;
        n++, p += len;
    }
    if (end) *end = p;
    return (p - BINCODE_TILE_BYTES) | n << 6;
}

// A walk across tiles: where it stands.  Composing maps is following them: the state after tiles [i, j) and the map of tile j give the
// state after [i, j].
struct BcChain {
    uint32_t entry;  // offset into the next tile (meaningless once stopped)
    uint32_t stopped;
    uint64_t records;  // whole records so far; stopped: the ordinal of the record that could not be read
};
BC_HD inline void bc_chain_step(BcChain& c, uint32_t map_entry) {
    if (c.stopped) return;
    c.records += map_entry >> 6;
    if ((map_entry & 63u) == BC_STOP) c.stopped = 1;
    else c.entry = map_entry & 63u;
}
// the same over a block of tiles: a block map entry is records | (exit or BC_STOP) << 32
BC_HD inline uint64_t bc_block_entry(const BcChain& c) { return c.records | (uint64_t)(c.stopped ? BC_STOP : c.entry) << 32; }
BC_HD inline void bc_chain_block(BcChain& c, uint64_t block_entry) {
    if (c.stopped) return;
    c.records += block_entry & 0xFFFFFFFFull;
    if ((uint32_t)(block_entry >> 32) == BC_STOP) c.stopped = 1;
    else c.entry = (uint32_t)(block_entry >> 32);
}

// ---- the decode ----
// The whole record (bc_peek's dom, opc) at offset p as the three 64-bit words of an rv_op (domain | opcode << 8 | dst << 32,
// a | b << 32, imm; reserved and unused fields zero), and the host parser's code for it: RV_E_BAD_OP for a bool that is not 0 / 1,
// else RV_E_UNSUPPORTED for a wire field above 2^32 - 1, else 0.
template <class R>
BC_HD inline int bc_decode(const R& r, uint32_t p, uint32_t dom, uint32_t opc, uint64_t w[3]) {
    const uint32_t f = bc_fields(dom, opc);
    uint32_t q = p + bc_head(dom);
    uint64_t dst = 0, a = 0, b = 0, imm = 0;
    if (f & BC_DST) dst = r.u64(q), q += 8;
    if (f & BC_A) a = r.u64(q), q += 8;
    if (f & BC_B) b = r.u64(q), q += 8;
    if (f & BC_IMM1) imm = r.u8(q);
    if (f & BC_IMM8) imm = r.u64(q);
    w[0] = (uint64_t)dom | (uint64_t)opc << 8 | (dst & 0xFFFFFFFFull) << 32;
    w[1] = (a & 0xFFFFFFFFull) | (b & 0xFFFFFFFFull) << 32;
    w[2] = imm;
    if ((f & BC_IMM1) && imm > 1) return RV_E_BAD_OP;
    if ((dst | a | b) >> 32) return RV_E_UNSUPPORTED;
    return 0;
}

// what a record adds to mcircuit::largest_wires (reverie_amd.ops.largest_wires): the wire counts it needs, 0 where it names none
BC_HD inline void bc_wire_needs(const uint64_t w[3], uint64_t& z64, uint64_t& gf2) {
    const uint32_t dom = (uint32_t)w[0] & 255u, opc = (uint32_t)(w[0] >> 8) & 255u;
    const uint64_t dst = w[0] >> 32, a = w[1] & 0xFFFFFFFFull, b = w[1] >> 32;
    z64 = gf2 = 0;
    if (dom == RV_DOM_B2A) z64 = dst + 1, gf2 = a + 64;
    else if (dom == RV_DOM_SIZEHINT) z64 = a, gf2 = b;
    else {
        const uint32_t f = bc_fields(dom, opc);
        uint64_t hi = 0;
        if ((f & BC_DST) && dst + 1 > hi) hi = dst + 1;
        if ((f & BC_A) && a + 1 > hi) hi = a + 1;
        if ((f & BC_B) && b + 1 > hi) hi = b + 1;
        (dom == RV_DOM_GF2 ? gf2 : z64) = hi;
    }
}

// ---- the writer ----
// the record's length in a file, 0 where the host writer returns RV_E_BAD_OP (reserved != 0, an unknown domain or opcode)
BC_HD inline uint32_t bc_op_len(const uint64_t w[3]) {
    const uint32_t dom = (uint32_t)w[0] & 255u, opc = (uint32_t)(w[0] >> 8) & 255u;
    if ((w[0] >> 16) & 0xFFFFu) return 0;
    if (dom >= BC_DOMAINS) return 0;
    if (bc_head(dom) != 8) return bc_record_len(dom, 0);  // (the opcode byte of such a record is not looked at, as the host's)
    return opc < BC_OPCODES ? bc_record_len(dom, opc) : 0;
}
// the record's bytes (bc_op_len of them, not 0) through put(offset, byte)
template <class Put>
BC_HD inline void bc_encode(const uint64_t w[3], Put put) {
    const uint32_t dom = (uint32_t)w[0] & 255u, opc = bc_head(dom) == 8 ? (uint32_t)(w[0] >> 8) & 255u : 0u;
    const uint32_t f = bc_fields(dom, opc);
    uint32_t q = 0;
    auto field = [&](uint64_t v, uint32_t bytes) {
        for (uint32_t k = 0; k < bytes; k++) put(q + k, (uint8_t)(v >> (8 * k)));
        q += bytes;
    };
    field(dom, 4);
    if (bc_head(dom) == 8) field(opc, 4);
    if (f & BC_DST) field(w[0] >> 32, 8);
    if (f & BC_A) field(w[1] & 0xFFFFFFFFull, 8);
    if (f & BC_B) field(w[1] >> 32, 8);
    if (f & BC_IMM1) field(w[2] & 1u, 1);
    if (f & BC_IMM8) field(w[2], 8);
}

// ---- windows ----
// One file of file_len bytes handed over in consecutive windows of any length (rv_program_reader_*: the rule is in
// include/reverie_amd.h, the stages in DESIGN §19.7).  Every record takes 16 .. 32 bytes, so what one window leaves the next is a
// file offset, the next ordinal and a carry of fewer than 32 bytes: the bytes behind the last whole record of the bytes fed so far.
// The 8 header bytes go through the same carry.  A window's kernels answer with a BcWindowResult; everything that decides -- what is
// carried, which stop is final, the offsets and the counts -- is the plain C++ below, which the CPU model of
// tests/bincode_window_model.cpp compiles as it stands.
constexpr uint64_t BC_NO_ERR = ~0ull;
enum { BC_I_GF2 = 0, BC_I_Z64, BC_I_B2A, BC_I_SIZEHINT, BC_I_Z64_WIRES, BC_I_GF2_WIRES, BC_I_IN_GF2, BC_I_IN_Z64, BC_I_WORDS };

// bytes in plain memory (the carry and the head of a window, put together)
struct BcBytes {
    const uint8_t* p;
    BC_HD uint32_t u8(uint32_t o) const { return p[o]; }
    BC_HD uint32_t u32(uint32_t o) const { return (uint32_t)p[o] | (uint32_t)p[o + 1] << 8 | (uint32_t)p[o + 2] << 16 | (uint32_t)p[o + 3] << 24; }
    BC_HD uint64_t u64(uint32_t o) const { return (uint64_t)u32(o) | (uint64_t)u32(o + 4) << 32; }
};

// The record that straddles into a window: r reads the carry's c bytes (1 .. 31) followed by the window's first avail - c bytes
// (up to 31 of them).  straddle = 1: the record is whole in those bytes; the window's walk enters at `entry` (< 32), w and code are
// bc_decode's.  straddle = 2: no record can be read there (bc_peek's 0) -- final when avail >= 32 or the file ends with the window.
struct BcEnter {
    uint32_t straddle, entry, dom;
    int code;
    uint64_t w[3];
};
template <class R>
BC_HD inline BcEnter bc_enter(const R& r, uint32_t c, uint32_t avail) {
    BcEnter e = {};
    uint32_t opc = 0;
    const uint32_t len = bc_peek(r, 0, avail, e.dom, opc);
    if (len <= c) {  // (0; a whole record is never left in the carry)
        e.straddle = 2;
        return e;
    }
    e.straddle = 1, e.entry = len - c;
    e.code = bc_decode(r, 0, e.dom, opc, e.w);
    return e;
}
// what a record adds to a window's info words
BC_HD inline bool bc_is_input(const uint64_t w[3], uint32_t dom) { return ((uint32_t)w[0] & 0xFFFFu) == dom; }  // (opcode RV_OP_INPUT = 0)

struct BcWindowState {
    uint64_t file_len, file_off;  // file_off: bytes fed so far
    uint64_t next_op, count;      // count: the header's, once have_count
    uint32_t have_count, open_count, carry_len, done;
    int code;                     // the first nonzero code: the reader is over
    uint8_t carry[BC_MAX_RECORD];
    rv_program_info info;
};
struct BcWindowLaunch {
    uint32_t carry_len, entry;  // carry_len != 0: the straddling record first; else the walk enters the window at `entry`
    uint64_t remaining;         // records the header still owes
};
struct BcWindowResult {
    uint32_t straddle;  // BcEnter's (0: there was no carry)
    uint64_t found;     // whole records in the carry and the window, the straddling one included
    uint64_t stop;      // the window offset the walk stopped at; BC_NO_ERR: it left the window at its last byte
    uint64_t err;       // the smallest ordinal (counted from the feed's first) << 8 | code among the records' own codes
    uint64_t bytes_end; // the window offset behind the record that is the header's last, where it is among them
    uint8_t tail[BC_MAX_RECORD];  // the window's bytes from `stop` on, where fewer than 32 (straddle == 2: the whole window)
    uint64_t info[BC_I_WORDS];
};

inline void bc_window_begin(BcWindowState& s, uint64_t file_len) {
    s = BcWindowState{};
    s.file_len = file_len;
}
// as if file_off bytes holding next_op whole records had been read; the count stays open: every whole record is delivered, and
// bc_window_finish closes it at the records delivered, where the bytes fed end with a record
inline void bc_window_resume(BcWindowState& s, uint64_t file_off, uint64_t next_op) {
    const uint64_t file_len = s.file_len;
    bc_window_begin(s, file_len);
    s.file_off = file_off, s.next_op = next_op, s.have_count = s.open_count = 1, s.count = ~0ull;
}
// bytes of the window's start the header still needs (0: the header is in)
inline uint32_t bc_window_head_need(const BcWindowState& s, uint64_t len) {
    if (s.have_count) return 0;
    const uint64_t need = BC_HEADER_BYTES - s.carry_len;
    return (uint32_t)(len < need ? len : need);
}
// those bytes.  -> 0, or the file's code (then the reader is over).  Without a count afterwards the feed is over (the whole window
// is in the carry); with one, the window is walked from offset n.
inline int bc_window_head(BcWindowState& s, const uint8_t* b, uint32_t n, uint64_t len) {
    if (s.file_len < BC_HEADER_BYTES) return s.code = RV_E_BAD_OP;
    for (uint32_t k = 0; k < n; k++) s.carry[s.carry_len++] = b[k];
    if (s.carry_len < BC_HEADER_BYTES) {
        s.file_off += len;  // (len == n)
        if (s.file_off == s.file_len) return s.code = RV_E_BAD_OP;
        return 0;
    }
    s.count = 0;
    for (uint32_t k = 0; k < BC_HEADER_BYTES; k++) s.count |= (uint64_t)s.carry[k] << (8 * k);
    if (s.count > (s.file_len - BC_HEADER_BYTES) / BC_MIN_RECORD) return s.code = RV_E_BAD_OP;
    s.have_count = 1, s.carry_len = 0;
    s.info.bytes = BC_HEADER_BYTES;
    if (!s.count) s.done = 1;
    return 0;
}
inline BcWindowLaunch bc_window_launch(const BcWindowState& s, uint32_t head_taken) {
    return BcWindowLaunch{s.carry_len, s.carry_len ? 0u : head_taken, s.count - s.next_op};
}
// a window of len bytes (none launched for: the records are all out, or len == 0)
inline void bc_window_skip(BcWindowState& s, uint64_t len, rv_program_piece* piece) {
    *piece = rv_program_piece{s.next_op, 0, 0, 0};
    s.file_off += len;
}
// what the window's kernels found -> the feed's code, the piece, the state behind the window
inline int bc_window_done(BcWindowState& s, uint64_t len, const BcWindowResult& res, rv_program_piece* piece) {
    const uint64_t remaining = s.count - s.next_op;
    const uint64_t deliver = res.found < remaining ? res.found : remaining;
    uint64_t err = res.err;
    uint32_t carry_len = 0;
    if (res.found < remaining) {
        // the walk stopped below the count: with 32 or more bytes before it, or at the file's end, no record can be read there
        const uint64_t stop = res.straddle == 2 ? 0 : res.stop == BC_NO_ERR ? len : res.stop;
        const uint64_t left = len - stop + (res.straddle == 2 ? s.carry_len : 0);
        // (an open count owes nothing: the file may end with a record)
        if (left >= BC_MAX_RECORD || (s.file_off + len == s.file_len && !(s.open_count && !left))) {
            const uint64_t e = res.found << 8 | (uint64_t)RV_E_BAD_OP;
            if (e < err) err = e;
        } else {
            carry_len = (uint32_t)left;
        }
    }
    if (err != BC_NO_ERR) return s.code = (int)(err & 0xFFu);
    const uint32_t keep = res.straddle == 2 ? s.carry_len : 0;  // (the carry grows by a window that completes no record)
    for (uint32_t k = keep; k < carry_len; k++) s.carry[k] = res.tail[k - keep];
    s.carry_len = carry_len;
    *piece = rv_program_piece{s.next_op, deliver, res.info[BC_I_IN_GF2], res.info[BC_I_IN_Z64]};
    rv_program_info& in = s.info;
    in.n_gf2 += res.info[BC_I_GF2], in.n_z64 += res.info[BC_I_Z64], in.n_b2a += res.info[BC_I_B2A], in.n_sizehint += res.info[BC_I_SIZEHINT];
    if (res.info[BC_I_Z64_WIRES] > in.z64_wires) in.z64_wires = res.info[BC_I_Z64_WIRES];
    if (res.info[BC_I_GF2_WIRES] > in.gf2_wires) in.gf2_wires = res.info[BC_I_GF2_WIRES];
    s.next_op += deliver;
    if (deliver && deliver == remaining) s.done = 1, in.bytes = s.file_off + res.bytes_end;
    else if (deliver) in.bytes = s.file_off + (res.straddle == 2 ? 0 : res.stop == BC_NO_ERR ? len : res.stop);
    s.file_off += len;
    return 0;
}
// RV_OK with the whole file's info once `count` records are out, RV_E_ARG before
inline int bc_window_finish(BcWindowState& s, rv_program_info* info) {
    if (s.code || !s.have_count) return RV_E_ARG;
    if (s.open_count && !s.carry_len) s.count = s.next_op, s.open_count = 0, s.done = 1;
    if (!s.done) return RV_E_ARG;
    s.info.n_ops = s.count;
    if (info) *info = s.info;
    return RV_OK;
}

}  // namespace rv

#if defined(__HIPCC__)
#include "compile_dev.h"

namespace rv {

struct BincodeRead {
    int code = 0;  // RV_OK, or the code of the first record (below the header's count) the host parser rejects
    rv_program_info info = {};
    bool written = false;
};
// d_data[0, len): the file in device memory (24 <= len < 2^32), count: its header's (1 <= count <= (len - 8) / 16).  d_ops: where the
// records go, room for `count` of them (null: nowhere).  Work memory from A, given back before the call returns; the stream is
// synchronised once, at the end.  RV_OK (res filled), RV_E_NOMEM or RV_E_DEVICE.
int bincode_read_device(hipStream_t st, const DevAlloc& A, const uint8_t* d_data, size_t len, uint64_t count, rv_op* d_ops, BincodeRead* res);
// One window of a file read in windows: d_data[0, len) (1 <= len < 2^32), the carry (launch.carry_len bytes) before it.  d_ops: room
// for len / 16 + 1 records (null: nowhere).  Work memory as above, by len; one synchronisation, at the end.
int bincode_window_device(hipStream_t st, const DevAlloc& A, const uint8_t* d_data, size_t len, const BcWindowLaunch& launch, const uint8_t* carry,
                          rv_op* d_ops, BcWindowResult* res);

struct BincodeWrite {
    int code = 0;        // RV_OK or RV_E_BAD_OP
    uint64_t bytes = 0;  // the file's length (with RV_OK)
    bool written = false;
};
// d_ops[0, n_ops) (n_ops < 2^28) as a file at d_out[0, cap) (null: nowhere); written only when there is no bad record and
// bytes <= min(cap, 2^32 - 1) -- decided on the device, one synchronisation.  header_count: the count the 8 header bytes say, in
// front of the records (a whole file: n_ops; the first feed of a file written in windows: the whole list's); null: the records alone.
int bincode_write_device(hipStream_t st, const DevAlloc& A, const rv_op* d_ops, size_t n_ops, uint8_t* d_out, uint64_t cap, const uint64_t* header_count,
                         BincodeWrite* res);

}  // namespace rv
#endif
