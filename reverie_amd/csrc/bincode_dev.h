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
template <class R>
BC_HD inline uint32_t bc_walk_tile(const R& r, uint32_t avail, uint32_t entry, uint16_t* starts) {
    uint32_t p = entry, n = 0, dom, opc;
    while (p < BINCODE_TILE_BYTES) {
        const uint32_t len = bc_peek(r, p, avail, dom, opc);
        if (!len) return BC_STOP | n << 6;
        if (starts) starts[n] = (uint16_t)p;
        n++, p += len;
    }
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

struct BincodeWrite {
    int code = 0;        // RV_OK or RV_E_BAD_OP
    uint64_t bytes = 0;  // the file's length (with RV_OK)
    bool written = false;
};
// d_ops[0, n_ops) (n_ops < 2^28) as a file at d_out[0, cap) (null: nowhere); written only when there is no bad record and
// bytes <= min(cap, 2^32 - 1) -- decided on the device, one synchronisation.
int bincode_write_device(hipStream_t st, const DevAlloc& A, const rv_op* d_ops, size_t n_ops, uint8_t* d_out, uint64_t cap, BincodeWrite* res);

}  // namespace rv
#endif
