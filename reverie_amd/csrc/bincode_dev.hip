// see bincode_dev.h
//
// A program file read by kernels.  Its records have six lengths, no delimiters and no alignment: where record i starts is known only
// once records 0 .. i - 1 have been read.  So the file is cut into tiles of BINCODE_TILE_BYTES, counted from data[0], and every tile
// is walked from every offset a record can enter it at (BC_ENTRIES = the longest record: 32).  No kernel waits for another workgroup;
// no byte at or behind data + len is read (stage_tile is the only code that reads the file).  The steps:
//   1. walk      a workgroup (one wavefront) stages its tile and the 31 bytes behind it, clipped to len, in LDS: aligned 16-byte loads
//                where the 16 bytes lie inside that range, bytes at its two ends.  Lanes 0 .. 31 walk from entries 0 .. 31: two tags, the
//                length from the layout table, a step -- until the position leaves the tile, or no record can be read at it (bc_peek:
//                an unknown tag, a record that passes len; the host parser has no length there either).  A lane leaves one 16-bit
//                map entry: its exit offset into the next tile or BC_STOP, and the records it started.
//   2. blocks    a tile's map sends an entry to (exit, records); following maps is associative.  A workgroup loads the maps of
//                BINCODE_SCAN_TILES tiles into LDS and 32 lanes chase their entry through them: the block's map.
//   3. chase     one workgroup follows the block maps from the true entry of tile 0 (offset 8, behind the header), 64 block maps in LDS
//                at a time, and leaves every block its true entry and first ordinal.  Where the chain stops is the first record that
//                cannot be read: RV_E_BAD_OP at that ordinal if it is below the header's count (so is the end of the data).
//   4. resolve   every block follows its tiles' maps again, now from its true entry: every tile's entry and first ordinal.
//   5. decode    a workgroup stages its tile again, one lane walks it from the true entry and lists the record starts, and all lanes
//                decode a record each: the rv_op as three 64-bit words into LDS, stored from there to d_ops in order (consecutive
//                lanes, consecutive words).  Ordinals at or behind the header's count are neither judged nor written.  The same pass
//                judges the fields (a bool above 1, a wire above 2^32 - 1: a 64-bit atomicMin of ordinal << 8 | code), counts the
//                domains and takes the wire maxima (LDS first, then one of 64 slots in device memory: few atomics per address).
// The first error is the smallest (ordinal, code) entered by 3 and 5; inside a record program.cpp decides RV_E_BAD_OP before
// RV_E_UNSUPPORTED, and so does bc_decode.  Records are written while the errors are still being found: with an error d_ops holds
// anything (the header allows it); whether they fit is known to the host before anything is launched (the count is the header's).
// Work memory: 64 bytes per tile for the maps and 8 for the entries (1.8 % of len), 256 bytes per block, the state words.
//
// A file read in windows (bincode_window_device) runs the same steps on one window, behind a step 0 (k_bc_enter) that
// decodes the record straddling in from the carry of the window before and hands the walk its entry; the whole file is the case "no
// carry, enter at offset 8".  The tile in which the chain stops leaves the stop's offset and the bytes behind it (the next carry);
// what is carried and which stop is final is decided on the host (bincode_dev.h: bc_window_*).
//
// A file written by kernels: 1. every record's length (0: a bad record) and their sum; 2. the exclusive scan of the lengths;
// 3. a workgroup lays its 256 records out in LDS, at the position modulo 16 their bytes have in d_out, and stores the image: 16-byte
// stores for the aligned chunks that are its own, bytes at the two ends (neighbours share those chunks).  Work memory: 4 bytes per record.
#include "bincode_dev.h"

#include <string.h>

#include <algorithm>
#include <vector>

namespace rv {
namespace {
#include "compile_dev_prims.inc"
[[maybe_unused]] const auto unused_sort = &radix_sort;  // (the scans are all this file takes from the building blocks)

constexpr uint32_t T = BINCODE_TILE_BYTES, B = BINCODE_SCAN_TILES, E = BC_ENTRIES;
constexpr int WAVE = 64;              // threads of the walk and decode workgroups
constexpr uint32_t RAW = T + 64;      // a tile's LDS image: up to 15 bytes of alignment, the tile, 31 bytes behind it, the readers' slack
constexpr uint32_t CHASE_BLOCKS = 64;  // block maps in LDS at a time
constexpr uint32_t SLOTS = 64;        // copies of the info words the decode workgroups spread their atomics over
// the state words: S_STOP, S_CHAIN0 (the chain the walk begins with: bc_block_entry), S_STRADDLE and S_TAIL are BcWindowResult's
enum {
    S_ERR, S_FOUND, S_BYTES, S_STOP, S_CHAIN0, S_STRADDLE, S_TAIL, S_INFO = S_TAIL + BC_MAX_RECORD / 8,
    I_GF2 = BC_I_GF2, I_Z64 = BC_I_Z64, I_B2A = BC_I_B2A, I_SIZEHINT = BC_I_SIZEHINT, I_Z64_WIRES = BC_I_Z64_WIRES, I_GF2_WIRES = BC_I_GF2_WIRES,
    I_IN_GF2 = BC_I_IN_GF2, I_IN_Z64 = BC_I_IN_Z64, I_WORDS = BC_I_WORDS, S_WORDS = S_INFO + SLOTS * I_WORDS
};
constexpr uint64_t NO_ERR = BC_NO_ERR;

// a tile's image in LDS: byte o of the tile is raw[sh + o]
struct LdsReader {
    const uint8_t* raw;  // 16-byte aligned
    uint32_t sh;
    __device__ uint32_t u8(uint32_t o) const { return raw[sh + o]; }
    __device__ uint32_t u32(uint32_t o) const {
        const uint32_t x = sh + o;
        const uint32_t* w = reinterpret_cast<const uint32_t*>(raw + (x & ~3u));
        return (uint32_t)(((uint64_t)w[1] << 32 | w[0]) >> (8 * (x & 3u)));
    }
    __device__ uint64_t u64(uint32_t o) const {
        const uint32_t x = sh + o, s = 8 * (x & 3u);
        const uint32_t* w = reinterpret_cast<const uint32_t*>(raw + (x & ~3u));
        const uint64_t lo = ((uint64_t)w[1] << 32 | w[0]) >> s, hi = ((uint64_t)w[2] << 32 | w[1]) >> s;
        return (lo & 0xFFFFFFFFull) | hi << 32;
    }
};
// data[tile * T, min(tile * T + T + 31, len)) into raw, by NT threads; -> the number of bytes (avail) and the image's shift
template <int NT>
__device__ inline uint32_t stage_tile(const uint8_t* data, uint64_t len, uint64_t tile, uint8_t* raw, uint32_t& sh) {
    const uint64_t lo = tile * T, hi = std::min<uint64_t>(lo + T + BC_MAX_RECORD - 1, len);
    const uint32_t avail = (uint32_t)(hi - lo);
    const uint8_t* g0 = data + lo;
    sh = (uint32_t)((uintptr_t)g0 & 15u);
    const uint8_t* base = g0 - sh;  // 16-byte aligned; the sh bytes before g0 are never read
    const uint32_t span = sh + avail;
    for (uint32_t c = threadIdx.x * 16; c < span; c += NT * 16) {
        if (c >= sh && c + 16 <= span) {
            *reinterpret_cast<uint4*>(raw + c) = *reinterpret_cast<const uint4*>(base + c);
        } else {
            for (uint32_t k = 0; k < 16; k++)
                if (c + k >= sh && c + k < span) raw[c + k] = base[c + k];
        }
    }
    __syncthreads();
    return avail;
}

// ---- the read ----
// The state words' first values and the chain the walk begins with.  c == 0: the walk enters the data at entry0.  c != 0 (a window
// behind a carry of c bytes): the record that straddles in is put together from the carry and the data's first bytes (tile 0,
// staged like any tile), decoded as ordinal 0 and written to out[0]; the walk enters behind it (bc_enter).
struct BcCarry {
    uint8_t b[BC_MAX_RECORD];
};
__global__ __launch_bounds__(TB) void k_bc_enter(const uint8_t* data, uint64_t len, BcCarry carry, uint32_t c, uint32_t entry0, uint64_t remaining,
                                                 uint64_t* out, uint64_t* state) {
    __shared__ __attribute__((aligned(16))) uint8_t raw[RAW];
    __shared__ uint8_t buf[2 * BC_MAX_RECORD];
    for (uint32_t k = threadIdx.x; k < S_WORDS; k += TB) state[k] = k == S_ERR || k == S_STOP ? NO_ERR : 0;
    __syncthreads();
    if (!c) {
        if (threadIdx.x == 0) state[S_CHAIN0] = bc_block_entry(BcChain{entry0, 0, 0});
        return;
    }
    uint32_t sh;
    const uint32_t avail = stage_tile<TB>(data, len, 0, raw, sh), m = std::min(avail, BC_MAX_RECORD - 1);
    if (threadIdx.x < c) buf[threadIdx.x] = carry.b[threadIdx.x];
    else if (threadIdx.x < c + m) buf[threadIdx.x] = raw[sh + threadIdx.x - c];
    __syncthreads();
    if (threadIdx.x) return;
    const BcEnter e = bc_enter(BcBytes{buf}, c, c + m);
    state[S_STRADDLE] = e.straddle;
    if (e.straddle == 2) {
        state[S_CHAIN0] = bc_block_entry(BcChain{0, 1, 0});
        state[S_STOP] = 0;
        uint8_t* tail = reinterpret_cast<uint8_t*>(&state[S_TAIL]);
        for (uint32_t k = 0; k < m; k++) tail[k] = buf[c + k];
        return;
    }
    state[S_CHAIN0] = bc_block_entry(BcChain{e.entry, 0, 1});
    if (e.code) state[S_ERR] = (uint64_t)e.code;
    else {
        uint64_t z, g;
        bc_wire_needs(e.w, z, g);
        uint64_t* w = &state[S_INFO];
        w[I_GF2 + e.dom] = 1, w[I_Z64_WIRES] = z, w[I_GF2_WIRES] = g;
        if (bc_is_input(e.w, RV_DOM_GF2)) w[I_IN_GF2] = 1;
        if (bc_is_input(e.w, RV_DOM_Z64)) w[I_IN_Z64] = 1;
    }
    if (remaining == 1) state[S_BYTES] = e.entry;
    if (out) out[0] = e.w[0], out[1] = e.w[1], out[2] = e.w[2];
}
__global__ __launch_bounds__(WAVE) void k_bc_walk(const uint8_t* data, uint64_t len, uint16_t* maps) {
    __shared__ __attribute__((aligned(16))) uint8_t raw[RAW];
    uint32_t sh;
    const uint32_t avail = stage_tile<WAVE>(data, len, blockIdx.x, raw, sh);
    if (threadIdx.x < E) maps[(size_t)blockIdx.x * E + threadIdx.x] = (uint16_t)bc_walk_tile(LdsReader{raw, sh}, avail, threadIdx.x, nullptr);
}

// the maps of block blk's tiles into sm (n of them)
__device__ inline uint32_t load_block_maps(const uint16_t* maps, uint32_t n_tiles, uint32_t blk, uint16_t* sm) {
    const uint32_t t0 = blk * B, n = std::min(B, n_tiles - t0);
    const uint32_t* src = reinterpret_cast<const uint32_t*>(maps + (size_t)t0 * E);
    uint32_t* dst = reinterpret_cast<uint32_t*>(sm);
    for (uint32_t k = threadIdx.x; k < n * E / 2; k += TB) dst[k] = src[k];
    __syncthreads();
    return n;
}
__global__ __launch_bounds__(TB) void k_bc_blocks(const uint16_t* maps, uint32_t n_tiles, uint64_t* bmaps) {
    __shared__ __attribute__((aligned(16))) uint16_t sm[B * E];
    const uint32_t n = load_block_maps(maps, n_tiles, blockIdx.x, sm);
    if (threadIdx.x >= E) return;
    BcChain c{threadIdx.x, 0, 0};
    for (uint32_t t = 0; t < n && !c.stopped; t++) bc_chain_step(c, sm[t * E + c.entry]);
    bmaps[(size_t)blockIdx.x * E + threadIdx.x] = bc_block_entry(c);
}
// block_in[b] = the chain before block b (bc_block_entry); the state words of the chain's end.  final: the data is a whole file --
// a chain that ends below the count is an error (of a window, the host decides: bc_window_done)
__global__ __launch_bounds__(TB) void k_bc_chase(const uint64_t* bmaps, uint32_t n_blocks, uint64_t count, int final, uint64_t* block_in, uint64_t* state) {
    __shared__ uint64_t sm[CHASE_BLOCKS * E];
    BcChain c{0, 0, 0};
    bc_chain_block(c, state[S_CHAIN0]);
    for (uint32_t b0 = 0; b0 < n_blocks; b0 += CHASE_BLOCKS) {
        const uint32_t n = std::min(CHASE_BLOCKS, n_blocks - b0);
        for (uint32_t k = threadIdx.x; k < n * E; k += TB) sm[k] = bmaps[(size_t)b0 * E + k];
        __syncthreads();
        if (threadIdx.x == 0)
            for (uint32_t b = 0; b < n; b++) {
                block_in[b0 + b] = bc_block_entry(c);
                if (!c.stopped) bc_chain_block(c, sm[b * E + c.entry]);
            }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        // stopped: record c.records cannot be read.  Not stopped: the chain left the last tile, which it can only do at the file's
        // last byte (a record that passes len stops it), and record c.records would begin at len.  RV_E_BAD_OP either way.
        state[S_FOUND] = c.records;
        if (final && c.records < count) state[S_ERR] = c.records << 8 | (uint64_t)RV_E_BAD_OP;
    }
}
__global__ __launch_bounds__(TB) void k_bc_resolve(const uint16_t* maps, uint32_t n_tiles, const uint64_t* block_in, uint64_t* tile_in) {
    __shared__ __attribute__((aligned(16))) uint16_t sm[B * E];
    const uint32_t n = load_block_maps(maps, n_tiles, blockIdx.x, sm);
    if (threadIdx.x) return;
    BcChain c{0, 0, 0};
    bc_chain_block(c, block_in[blockIdx.x]);
    for (uint32_t t = 0; t < n; t++) {
        tile_in[(size_t)blockIdx.x * B + t] = bc_block_entry(c);
        if (!c.stopped) bc_chain_step(c, sm[t * E + c.entry]);
    }
}

__global__ __launch_bounds__(WAVE) void k_bc_decode(const uint8_t* data, uint64_t len, const uint64_t* tile_in, uint64_t count, uint64_t* out,
                                                    uint64_t* state) {
    __shared__ __attribute__((aligned(16))) uint8_t raw[RAW];
    __shared__ uint16_t starts[BC_TILE_RECORDS];
    __shared__ uint64_t words[WAVE * 3];
    __shared__ uint32_t n_found;
    __shared__ unsigned long long acc[I_WORDS];
    const uint64_t in = tile_in[blockIdx.x];
    const uint64_t first = in & 0xFFFFFFFFull;  // the ordinal of the tile's first record
    if ((uint32_t)(in >> 32) == BC_STOP || first >= count) return;
    uint32_t sh;
    const uint32_t avail = stage_tile<WAVE>(data, len, blockIdx.x, raw, sh);
    const LdsReader r{raw, sh};
    if (threadIdx.x < I_WORDS) acc[threadIdx.x] = 0;
    if (threadIdx.x == 0) {
        uint32_t end;
        const uint32_t m = bc_walk_tile(r, avail, (uint32_t)(in >> 32), starts, &end);
        n_found = m >> 6;
        if ((m & 63u) == BC_STOP) {  // the one tile the chain stops in: where, and the bytes from there on where they end the data
            state[S_STOP] = (uint64_t)blockIdx.x * T + end;
            if ((uint64_t)blockIdx.x * T + avail == len && avail - end < BC_MAX_RECORD) {
                uint8_t* tail = reinterpret_cast<uint8_t*>(&state[S_TAIL]);
                for (uint32_t k = end; k < avail; k++) tail[k - end] = (uint8_t)r.u8(k);
            }
        }
    }
    __syncthreads();
    const uint32_t n = (uint32_t)std::min<uint64_t>(n_found, count - first);
    uint32_t cnt[4] = {0, 0, 0, 0}, inputs[2] = {0, 0};
    uint64_t z64 = 0, gf2 = 0;
    for (uint32_t r0 = 0; r0 < n; r0 += WAVE) {
        const uint32_t i = r0 + threadIdx.x;
        if (i < n) {
            uint32_t dom = 0, opc = 0;
            const uint32_t p = starts[i], rec_len = bc_peek(r, p, avail, dom, opc);  // (not 0: the walk took this record)
            uint64_t w[3];
            const int code = bc_decode(r, p, dom, opc, w);
            if (code) atomicMin((unsigned long long*)&state[S_ERR], (unsigned long long)((first + i) << 8 | (uint64_t)code));
            else {
                uint64_t z, g;
                bc_wire_needs(w, z, g);
                cnt[dom]++, z64 = std::max(z64, z), gf2 = std::max(gf2, g);
                if (dom < 2 && opc == RV_OP_INPUT) inputs[dom]++;
            }
            if (first + i == count - 1) state[S_BYTES] = (uint64_t)blockIdx.x * T + p + rec_len;
            words[threadIdx.x * 3] = w[0], words[threadIdx.x * 3 + 1] = w[1], words[threadIdx.x * 3 + 2] = w[2];
        }
        __syncthreads();
        if (out) {
            const uint32_t m = std::min<uint32_t>(WAVE, n - r0) * 3;
            uint64_t* dst = out + (first + r0) * 3;
            for (uint32_t j = threadIdx.x; j < m; j += WAVE) dst[j] = words[j];
        }
        __syncthreads();
    }
    for (int d = 0; d < 4; d++)
        if (cnt[d]) atomicAdd(&acc[I_GF2 + d], (unsigned long long)cnt[d]);
    for (int d = 0; d < 2; d++)
        if (inputs[d]) atomicAdd(&acc[I_IN_GF2 + d], (unsigned long long)inputs[d]);
    if (z64) atomicMax(&acc[I_Z64_WIRES], (unsigned long long)z64);
    if (gf2) atomicMax(&acc[I_GF2_WIRES], (unsigned long long)gf2);
    __syncthreads();
    if (threadIdx.x < I_WORDS && acc[threadIdx.x]) {
        unsigned long long* slot = (unsigned long long*)&state[S_INFO + (blockIdx.x % SLOTS) * I_WORDS + threadIdx.x];
        if (threadIdx.x == I_Z64_WIRES || threadIdx.x == I_GF2_WIRES) atomicMax(slot, acc[threadIdx.x]);
        else atomicAdd(slot, acc[threadIdx.x]);
    }
}

// ---- the write ----
enum { W_BAD, W_TOTAL, W_WORDS };
__device__ inline void load_op(const uint64_t* ops, uint64_t i, uint64_t w[3]) { w[0] = ops[i * 3], w[1] = ops[i * 3 + 1], w[2] = ops[i * 3 + 2]; }
__global__ __launch_bounds__(TB) void k_bw_lens(const uint64_t* ops, uint64_t n, uint32_t* lens, uint64_t* state) {
    __shared__ unsigned int sum;
    if (threadIdx.x == 0) sum = 0;
    __syncthreads();
    const uint64_t i = (uint64_t)blockIdx.x * TB + threadIdx.x;
    if (i < n) {
        uint64_t w[3];
        load_op(ops, i, w);
        const uint32_t l = bc_op_len(w);
        lens[i] = l;
        if (!l) state[W_BAD] = 1;
        atomicAdd(&sum, l);
    }
    __syncthreads();
    if (threadIdx.x == 0) atomicAdd((unsigned long long*)&state[W_TOTAL], (unsigned long long)sum);
}
// HEADER: the image of block 0 begins with `count` as the file's header (a whole file: n; the first feed of a file written in windows:
// the whole list's count); else the records alone (a later feed)
template <bool HEADER>
__global__ __launch_bounds__(TB) void k_bw_emit(const uint64_t* ops, uint64_t n, const uint32_t* offs, const uint64_t* state, uint64_t cap, uint64_t count,
                                                uint8_t* out) {
    constexpr uint32_t head = HEADER ? BC_HEADER_BYTES : 0;
    __shared__ __attribute__((aligned(16))) uint8_t raw[16 + TB * BC_MAX_RECORD + 16];
    __shared__ uint64_t s_end;
    if (state[W_BAD] || head + state[W_TOTAL] > cap) return;
    const uint64_t first = (uint64_t)blockIdx.x * TB, i = first + threadIdx.x;
    const uint32_t mine = (uint32_t)std::min<uint64_t>(TB, n > first ? n - first : 0);
    // the block's bytes: d_out[g0, g1); block 0's begin with the header
    const uint64_t g0 = blockIdx.x ? head + (uint64_t)offs[first] : 0;
    const uint32_t sh = (uint32_t)((uintptr_t)(out + g0) & 15u);
    if (threadIdx.x == 0 && mine == 0) s_end = head;  // (no record: the header alone)
    if (blockIdx.x == 0 && threadIdx.x == 0)
        for (uint32_t k = 0; k < head; k++) raw[sh + k] = (uint8_t)(count >> (8 * k));
    if (threadIdx.x < mine) {
        uint64_t w[3];
        load_op(ops, i, w);
        const uint64_t at = head + (uint64_t)offs[i];
        uint8_t* dst = raw + sh + (uint32_t)(at - g0);
        bc_encode(w, [&](uint32_t k, uint8_t v) { dst[k] = v; });
        if (threadIdx.x == mine - 1) s_end = at + bc_op_len(w);
    }
    __syncthreads();
    const uint32_t span = sh + (uint32_t)(s_end - g0);
    uint8_t* base = out + g0 - sh;  // 16-byte aligned; only [sh, span) of it is this block's to write
    for (uint32_t c = threadIdx.x * 16; c < span; c += TB * 16) {
        if (c >= sh && c + 16 <= span) {
            *reinterpret_cast<uint4*>(base + c) = *reinterpret_cast<const uint4*>(raw + c);
        } else {
            for (uint32_t k = 0; k < 16; k++)
                if (c + k >= sh && c + k < span) base[c + k] = raw[c + k];
        }
    }
}

}  // namespace

// the five steps over d_data[0, len), entered as k_bc_enter says; `count` records at the most are judged and written; h: the state words
static int read_steps(hipStream_t st, const DevAlloc& A, const uint8_t* d_data, size_t len, const BcCarry& carry, uint32_t c, uint32_t entry0,
                      uint64_t count, int final, rv_op* d_ops, std::vector<uint64_t>& h) {
    Scratch S(A, st);
    const uint32_t n_tiles = blocks(len, T), n_blocks = blocks(n_tiles, B);
    uint64_t* state = S.get<uint64_t>(S_WORDS);
    uint16_t* maps = S.get<uint16_t>((size_t)n_tiles * E);
    uint64_t *bmaps = S.get<uint64_t>((size_t)n_blocks * E), *block_in = S.get<uint64_t>(n_blocks), *tile_in = S.get<uint64_t>((size_t)n_blocks * B);
    CDNEED(state && maps && bmaps && block_in && tile_in);

    uint64_t* out = reinterpret_cast<uint64_t*>(d_ops);
    k_bc_enter<<<1, TB, 0, st>>>(d_data, len, carry, c, entry0, count, out, state);
    k_bc_walk<<<n_tiles, WAVE, 0, st>>>(d_data, len, maps);
    k_bc_blocks<<<n_blocks, TB, 0, st>>>(maps, n_tiles, bmaps);
    k_bc_chase<<<1, TB, 0, st>>>(bmaps, n_blocks, count, final, block_in, state);
    k_bc_resolve<<<n_blocks, TB, 0, st>>>(maps, n_tiles, block_in, tile_in);
    k_bc_decode<<<n_tiles, WAVE, 0, st>>>(d_data, len, tile_in, count, out, state);
    CDCHK(hipGetLastError());
    h.resize(S_WORDS);
    CDCHK(fetch(st, h, state));
    CDCHK(hipStreamSynchronize(st));
    return RV_OK;
}

int bincode_read_device(hipStream_t st, const DevAlloc& A, const uint8_t* d_data, size_t len, uint64_t count, rv_op* d_ops, BincodeRead* res) {
    std::vector<uint64_t> h;
    if (int rc = read_steps(st, A, d_data, len, BcCarry{}, 0, BC_HEADER_BYTES, count, 1, d_ops, h)) return rc;
    *res = BincodeRead{};
    if (h[S_ERR] != NO_ERR) {
        res->code = (int)(h[S_ERR] & 0xFFu);
        return RV_OK;
    }
    rv_program_info& in = res->info;
    in.n_ops = count, in.bytes = h[S_BYTES];
    for (uint32_t s = 0; s < SLOTS; s++) {
        const uint64_t* w = &h[S_INFO + s * I_WORDS];
        in.n_gf2 += w[I_GF2], in.n_z64 += w[I_Z64], in.n_b2a += w[I_B2A], in.n_sizehint += w[I_SIZEHINT];
        in.z64_wires = std::max(in.z64_wires, w[I_Z64_WIRES]), in.gf2_wires = std::max(in.gf2_wires, w[I_GF2_WIRES]);
    }
    res->written = d_ops != nullptr;
    return RV_OK;
}

int bincode_window_device(hipStream_t st, const DevAlloc& A, const uint8_t* d_data, size_t len, const BcWindowLaunch& launch, const uint8_t* carry,
                          rv_op* d_ops, BcWindowResult* res) {
    BcCarry cb = {};
    memcpy(cb.b, carry, launch.carry_len);
    std::vector<uint64_t> h;
    if (int rc = read_steps(st, A, d_data, len, cb, launch.carry_len, launch.entry, launch.remaining, 0, d_ops, h)) return rc;
    *res = BcWindowResult{};
    res->straddle = (uint32_t)h[S_STRADDLE], res->found = h[S_FOUND], res->stop = h[S_STOP], res->err = h[S_ERR], res->bytes_end = h[S_BYTES];
    memcpy(res->tail, &h[S_TAIL], BC_MAX_RECORD);
    for (uint32_t s = 0; s < SLOTS; s++) {
        const uint64_t* w = &h[S_INFO + s * I_WORDS];
        for (uint32_t k = 0; k < I_WORDS; k++)
            if (k == I_Z64_WIRES || k == I_GF2_WIRES) res->info[k] = std::max(res->info[k], w[k]);
            else res->info[k] += w[k];
    }
    return RV_OK;
}

int bincode_write_device(hipStream_t st, const DevAlloc& A, const rv_op* d_ops, size_t n_ops, uint8_t* d_out, uint64_t cap, const uint64_t* header_count,
                         BincodeWrite* res) {
    Scratch S(A, st);
    uint64_t* state = S.get<uint64_t>(W_WORDS);
    uint32_t* lens = S.get<uint32_t>(n_ops);
    CDNEED(state && lens);
    const uint64_t* ops = reinterpret_cast<const uint64_t*>(d_ops);
    const uint32_t grid = blocks(n_ops, TB);
    const uint64_t room = std::min<uint64_t>(cap, 0xFFFFFFFFull);
    const uint32_t head = header_count ? BC_HEADER_BYTES : 0;

    CDCHK(hipMemsetAsync(state, 0, W_WORDS * 8, st));
    if (n_ops) {
        k_bw_lens<<<grid, TB, 0, st>>>(ops, n_ops, lens, state);
        CDCHK(hipGetLastError());
        CDCHK((scan_excl<uint32_t, SumU32>(S, st, lens, lens, n_ops, nullptr)));  // (wraps only where nothing is written)
    }
    if (d_out && header_count) k_bw_emit<true><<<grid, TB, 0, st>>>(ops, n_ops, lens, state, room, *header_count, d_out);
    else if (d_out) k_bw_emit<false><<<grid, TB, 0, st>>>(ops, n_ops, lens, state, room, 0, d_out);
    CDCHK(hipGetLastError());
    std::vector<uint64_t> h(W_WORDS);
    CDCHK(fetch(st, h, state));
    CDCHK(hipStreamSynchronize(st));
    *res = BincodeWrite{};
    if (h[W_BAD]) {
        res->code = RV_E_BAD_OP;
        return RV_OK;
    }
    res->bytes = head + h[W_TOTAL];
    res->written = d_out && res->bytes <= room;
    return RV_OK;
}
#undef CDCHK
#undef CDNEED

}  // namespace rv
