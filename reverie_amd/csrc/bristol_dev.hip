// see bristol_dev.h
//
// The gate lines of a Bristol text, parsed by kernels built from the device compiler's blocks (compile_dev_prims.inc: the scans,
// Scratch).  No kernel waits for another workgroup; no byte at or behind text + len is read.  The steps:
//   1. tiles      every workgroup takes BRISTOL_TILE_BYTES of the gate region, 16 bytes per lane (one 16-byte load where the 16 bytes lie
//                 inside the region, bytewise at its two ends), and classifies them: LF, whitespace (space, tab, CR), token byte.  A
//                 gate line is counted where its FIRST TOKEN BYTE lies: a token byte with nothing but whitespace between it and the
//                 LF before it.  Whether a tile begins inside a line that already has a token is not known to the tile: it counts as
//                 if not, and says whether its first count depends on it.  The flag itself is an exclusive max-scan over the tiles of
//                 (tile + 1) << 1 | "a token follows the tile's last LF" for the tiles that hold anything but whitespace (a line may
//                 span any number of tiles); the corrected counts' exclusive sum gives every tile its first line index.
//   2. lines      the same classification again, now with the flag: the offset (u32) of the first token byte of gate lines
//                 0 .. n_gates - 1; lines beyond are dropped.
//   3. validate   one thread per line walks its tokens once with constant state (so a MAND line of any length costs O(tokens)): every
//                 token is read as a number by the host's rule while the walk does not yet know whether it is the last one (the kind);
//                 the line's code by the host's order of decisions, its record count (1; nout for MAND) and its class.  The first
//                 error is one 64-bit atomicMin of line << 8 | code; a short file enters the same word at line = lines found.
//   4. emit       the exclusive sum of the record counts is each line's first record.  One thread per line walks the line again;
//                 a MAND line of more than one lane with three cursors in step (in[k], in[nout + k], out[k]).  Inputs and the
//                 assertion pairs are a thread per record.  Every record is three 8-byte stores: no byte is left unwritten.
//                 The emit kernels look at the error word and the capacity themselves, so the host synchronises once, at the end.
// Work memory: 8 bytes per gate line the call can judge (the lines still due, and no more than bytes / 8 + 2: br_line_cap), 8 bytes
// per tile and the scans' sums.
//
// A window of a reader (rv_bristol_reader_*) runs the same kernels on one buffer -- the carry, then the window -- that
// begins at a line's start; the whole text is the window that has no carry and ends the file.  What a lane and a line do is in
// bristol_dev.h (host-and-device functions the CPU model shares).  A window adds: the lines judged are the FINAL ones (BrTake: the
// line behind the last LF is left out unless the file ends here), cut off at the lines still due -- both decided on the device from
// the state words, so nothing is fetched in between; the offset behind the last LF, a maximum per tile in LDS and over the tiles in a
// state word, which tells the host what to carry; the short-file rule only where the file ends; the Input and assertion kernels
// only in their feeds; a record's place relative to the piece.  Line numbers, ordinals and class totals live on the host, 64-bit.
#include "bristol_dev.h"

#include <algorithm>
#include <vector>

namespace rv {
namespace {
#include "compile_dev_prims.inc"
[[maybe_unused]] const auto unused_sort = &radix_sort;  // (the scans are all this file takes from the building blocks)
static_assert(TB * 16 == BRISTOL_TILE_BYTES, "a lane takes 16 bytes of a tile");
static_assert(TB == BRISTOL_WG_LINES, "a thread per line");

// the words of one call in device memory (64-bit each): the first error, the first token bytes found, the records of the lines judged,
// their classes, the tiles' last scan key (bit 0: a token follows the last LF), the offset behind the last LF (a window's)
enum { S_ERR, S_LINES, S_OPS, S_AND, S_XOR, S_INV, S_OTHER, S_TAIL, S_LFEND, S_WORDS };
constexpr uint64_t NO_ERR = ~0ull;

// the lines this call judges: the final ones (BrTake), as far as the line table goes
struct Take {
    BrTake t;
    uint64_t n;
};
__device__ inline Take take_of(const uint64_t* state, bool at_end, uint64_t want, uint64_t cap) {
    Take r;
    r.t = br_take(state[S_LINES], (uint32_t)state[S_TAIL], at_end, want);
    r.n = r.t.take < cap ? r.t.take : cap;
    return r;
}

// ---- steps 1 and 2 ----
// the 16 bytes at c that lie in [lo, hi): bit k of lf / tok = byte k is a line feed / a token byte
__device__ inline void classify16(const uint8_t* c, const uint8_t* lo, const uint8_t* hi, uint32_t& lf, uint32_t& tok) {
    lf = tok = 0;
    if (c >= hi || c + 16 <= lo) return;
    if (c >= lo && c + 16 <= hi) {  // (c is 16-byte aligned: the tiles start at an aligned address)
        const uint4 v = *reinterpret_cast<const uint4*>(c);
        const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int k = 0; k < 16; k++) br_class((w[k >> 2] >> (8 * (k & 3))) & 255u, k, lf, tok);
    } else {
        br_classify_bytes(c, lo, hi, lf, tok);
    }
}
// LINES false: tkey[t] = the tile's scan key, tmeta[t] = its line count had it begun at a line's start | bit 31: the first of them is
// no line start when the tile begins inside a line with a token; WINDOW: the offset behind the text's last LF, a maximum over the lanes
// of a tile in LDS and over the tiles in state[S_LFEND].  LINES true: tin = the keys' exclusive max-scan, tbase = the first line index of
// every tile; the line table, cut off at the lines this call judges (take_of).
template <bool LINES, bool WINDOW>
__global__ __launch_bounds__(TB) void k_bp_tiles(const uint8_t* text, const uint8_t* base, const uint8_t* lo, const uint8_t* hi, uint32_t* tkey,
                                                 uint32_t* tmeta, const uint32_t* tin, const uint32_t* tbase, uint64_t* state, uint64_t want, uint64_t cap,
                                                 bool at_end, uint32_t* line_off) {
    __shared__ uint32_t sh[TB];
    __shared__ uint32_t cond, lf_end;
    if (threadIdx.x == 0) cond = 0, lf_end = 0;
    const uint8_t* c = base + (size_t)blockIdx.x * BRISTOL_TILE_BYTES + (size_t)threadIdx.x * 16;
    uint32_t lf, tok;
    classify16(c, lo, hi, lf, tok);
    // the state a lane begins in: the flag of the last lane before it that holds anything but whitespace, else the tile's
    const uint32_t key = br_lane_key(threadIdx.x, lf, tok);
    uint32_t last;
    const uint32_t prev = block_excl<uint32_t, MaxU32>(key, sh, &last);  // (its barriers order the two words' initialisation, too)
    const uint32_t tile_in = LINES ? (tin[blockIdx.x] & 1u) : 0u;
    const uint32_t starts = br_lane_starts(lf, tok, prev ? (prev & 1u) : tile_in);
    if (!LINES && !prev && (lf | tok)) cond = br_lane_cond(lf, tok);  // (one lane at most: the first with content)
    if (WINDOW && lf) atomicMax(&lf_end, br_lane_lf_end(lf, (uint64_t)(c - text)));
    uint32_t total;
    const uint32_t ex = block_excl<uint32_t, SumU32>(__popc(starts), sh, &total);
    if (!LINES) {
        if (threadIdx.x == 0) {
            tkey[blockIdx.x] = br_tile_key(blockIdx.x, last);
            tmeta[blockIdx.x] = total | (cond << 31);
            if (WINDOW && lf_end) atomicMax((unsigned long long*)&state[S_LFEND], (unsigned long long)lf_end);
        }
    } else {
        const uint64_t n = take_of(state, at_end, want, cap).n;
        uint64_t idx = (uint64_t)tbase[blockIdx.x] + ex;
        for (int k = 0; k < 16 && idx < n; k++)
            if ((starts >> k) & 1u) line_off[idx++] = (uint32_t)(c + k - text);
    }
}
__global__ __launch_bounds__(TB) void k_bp_counts(const uint32_t* tin, uint32_t* tmeta, uint32_t n_tiles) {
    const uint32_t t = blockIdx.x * TB + threadIdx.x;
    if (t >= n_tiles) return;
    tmeta[t] = br_tile_count(tmeta[t], tin[t]);
}

// ---- steps 3 and 4 (what a line needs: bristol_dev.h) ----
__global__ __launch_bounds__(TB) void k_bp_validate(const uint8_t* text, const uint8_t* hi, const uint32_t* line_off, uint64_t want, uint64_t cap, bool at_end,
                                                    uint64_t n_wires, uint32_t* cnt, uint64_t* state) {
    __shared__ unsigned long long cls[4];  // and, xor, inv, other
    if (threadIdx.x < 4) cls[threadIdx.x] = 0;
    __syncthreads();
    const uint64_t i = (uint64_t)blockIdx.x * TB + threadIdx.x;
    const Take tk = take_of(state, at_end, want, cap);
    BrLine r{0, -1, 0};
    if (i < tk.n) r = br_validate(text + line_off[i], hi, n_wires);
    else if (tk.t.short_file && i == tk.t.found) r.code = RV_E_BAD_OP;  // the file is short: the host fails at the first line it cannot read
    if (i < cap) cnt[i] = (uint32_t)r.recs;
    if (r.code) atomicMin((unsigned long long*)&state[S_ERR], (unsigned long long)(i << 8 | (uint64_t)r.code));
    else if (r.cl >= 0) atomicAdd(&cls[r.cl], (unsigned long long)r.recs);
    __syncthreads();
    if (threadIdx.x < 4 && cls[threadIdx.x]) atomicAdd((unsigned long long*)&state[S_AND + threadIdx.x], cls[threadIdx.x]);
}

// what the emit kernels are given beside the text: the piece is n_inputs Input records, the lines' records, then (with the last line)
// n_pairs assertion pairs; a record's place is relative to the piece
struct Emit {
    uint64_t want, cap;  // BrTake's want, the line table's length
    bool at_end;
    uint64_t n_inputs, n_pairs, cap_ops;
};
// the records are written when the text has no error and they fit
__device__ inline bool emit_wanted(const uint64_t* state, const Emit& e, Take& tk) {
    tk = take_of(state, e.at_end, e.want, e.cap);
    return state[S_ERR] == NO_ERR && e.n_inputs + state[S_OPS] + (tk.t.last ? 2 * e.n_pairs : 0) <= e.cap_ops;
}
__global__ __launch_bounds__(TB) void k_bp_emit(const uint8_t* text, const uint8_t* hi, const uint32_t* line_off, const uint32_t* first, const uint64_t* state,
                                                Emit e, uint64_t* out) {
    Take tk;
    if (!emit_wanted(state, e, tk)) return;
    const uint64_t i = (uint64_t)blockIdx.x * TB + threadIdx.x;
    if (i >= tk.n) return;
    br_emit(text + line_off[i], hi, out, e.n_inputs + first[i]);
}
__global__ __launch_bounds__(TB) void k_bp_inputs(const uint64_t* state, Emit e, uint64_t* out) {
    Take tk;
    if (!emit_wanted(state, e, tk)) return;
    for (uint64_t w = (uint64_t)blockIdx.x * TB + threadIdx.x; w < e.n_inputs; w += (uint64_t)gridDim.x * TB) br_emit_input(out, w, w);
}
__global__ __launch_bounds__(TB) void k_bp_asserts(const uint64_t* state, Emit e, uint64_t n_wires, const uint8_t* expected, uint64_t* out) {
    Take tk;
    if (!emit_wanted(state, e, tk) || !tk.t.last) return;
    const uint64_t k = (uint64_t)blockIdx.x * TB + threadIdx.x;
    if (k >= e.n_pairs) return;
    br_emit_pair(out, e.n_inputs + state[S_OPS] + 2 * k, n_wires, e.n_pairs, k, expected[k]);
}

// The steps on text[lo, hi) (lo at a line's start; offsets in the line table count from text).  h receives the words.
int gates_run(hipStream_t st, const DevAlloc& A, const uint8_t* text, const uint8_t* lo, const uint8_t* hi, const BrWindowLaunch& l, bool window,
              uint64_t n_wires, const uint8_t* d_expected, rv_op* d_ops, uint64_t cap_ops, std::vector<uint64_t>& h) {
    Scratch S(A, st);
    const uint8_t* base = lo - ((uintptr_t)lo & 15);  // (bytes before lo are never read: classify16)
    const uint32_t n_tiles = blocks((size_t)(hi - base), BRISTOL_TILE_BYTES);
    const uint64_t cap = br_line_cap((uint64_t)(hi - lo), l.want);
    uint64_t* state = S.get<uint64_t>(S_WORDS);
    uint32_t *tkey = S.get<uint32_t>(n_tiles), *tmeta = S.get<uint32_t>(n_tiles);
    uint32_t *line_off = S.get<uint32_t>(cap), *cnt = S.get<uint32_t>(cap);
    CDNEED(state && tkey && tmeta && line_off && cnt);
    const uint32_t gl = blocks(cap, TB);

    CDCHK(hipMemsetAsync(state, 0, S_WORDS * 8, st));
    CDCHK(hipMemsetAsync(state, 0xFF, 8, st));
    if (window) k_bp_tiles<false, true><<<n_tiles, TB, 0, st>>>(text, base, lo, hi, tkey, tmeta, nullptr, nullptr, state, l.want, cap, l.at_end, nullptr);
    else k_bp_tiles<false, false><<<n_tiles, TB, 0, st>>>(text, base, lo, hi, tkey, tmeta, nullptr, nullptr, state, l.want, cap, l.at_end, nullptr);
    CDCHK(hipGetLastError());
    CDCHK((scan_excl<uint32_t, MaxU32>(S, st, tkey, tkey, n_tiles, (uint32_t*)&state[S_TAIL])));
    k_bp_counts<<<blocks(n_tiles, TB), TB, 0, st>>>(tkey, tmeta, n_tiles);
    CDCHK((scan_excl<uint32_t, SumU32>(S, st, tmeta, tmeta, n_tiles, (uint32_t*)&state[S_LINES])));
    k_bp_tiles<true, false><<<n_tiles, TB, 0, st>>>(text, base, lo, hi, nullptr, nullptr, tkey, tmeta, state, l.want, cap, l.at_end, line_off);
    k_bp_validate<<<gl, TB, 0, st>>>(text, hi, line_off, l.want, cap, l.at_end, n_wires, cnt, state);
    CDCHK(hipGetLastError());
    CDCHK((scan_excl<uint32_t, SumU32>(S, st, cnt, cnt, cap, (uint32_t*)&state[S_OPS])));
    if (d_ops) {
        uint64_t* out = reinterpret_cast<uint64_t*>(d_ops);
        const Emit e{l.want, cap, l.at_end, l.n_inputs, l.n_pairs, cap_ops};
        k_bp_emit<<<gl, TB, 0, st>>>(text, hi, line_off, cnt, state, e, out);
        if (l.n_inputs) k_bp_inputs<<<std::min<uint32_t>(blocks(l.n_inputs, TB), 1u << 16), TB, 0, st>>>(state, e, out);
        if (l.n_pairs) k_bp_asserts<<<blocks(l.n_pairs, TB), TB, 0, st>>>(state, e, n_wires, d_expected, out);
        CDCHK(hipGetLastError());
    }
    h.assign(S_WORDS, 0);
    CDCHK(fetch(st, h, state));
    CDCHK(hipStreamSynchronize(st));
    return RV_OK;
}

}  // namespace

int bristol_gates_device(hipStream_t st, const DevAlloc& A, const uint8_t* d_text, size_t len, size_t gates_offset, uint64_t n_gates, uint64_t n_wires,
                         uint64_t n_inputs, const uint8_t* d_expected, uint64_t n_pairs, rv_op* d_ops, uint64_t cap_ops, BristolGates* res) {
    std::vector<uint64_t> h;
    const BrWindowLaunch l{n_gates, n_inputs, n_pairs, true};  // (the whole text is one window that reaches the file's end)
    if (const int rc = gates_run(st, A, d_text, d_text + gates_offset, d_text + len, l, false, n_wires, d_expected, d_ops, cap_ops, h)) return rc;
    *res = BristolGates{};
    if (h[S_ERR] != NO_ERR) {
        res->code = (int)(h[S_ERR] & 0xFFu);
        return RV_OK;
    }
    res->gate_ops = h[S_OPS];
    res->n_and = h[S_AND], res->n_xor = h[S_XOR], res->n_inv = h[S_INV], res->n_other = h[S_OTHER];
    res->written = d_ops && n_inputs + h[S_OPS] + 2 * n_pairs <= cap_ops;
    return RV_OK;
}

int bristol_window_device(hipStream_t st, const DevAlloc& A, const uint8_t* d_buf, size_t bytes, const BrWindowLaunch& l, uint64_t n_wires,
                          const uint8_t* d_expected, rv_op* d_ops, uint64_t cap_ops, BrWindowResult* res) {
    std::vector<uint64_t> h;
    if (const int rc = gates_run(st, A, d_buf, d_buf, d_buf + bytes, l, true, n_wires, d_expected, d_ops, cap_ops, h)) return rc;
    *res = BrWindowResult{};
    if (h[S_ERR] != NO_ERR) {
        res->code = (int)(h[S_ERR] & 0xFFu);
        return RV_OK;
    }
    const BrTake t = br_take(h[S_LINES], (uint32_t)h[S_TAIL], l.at_end, l.want);
    res->n_lines = t.take, res->last = t.last;
    res->gate_ops = h[S_OPS];
    res->n_and = h[S_AND], res->n_xor = h[S_XOR], res->n_inv = h[S_INV], res->n_other = h[S_OTHER];
    res->carry_from = h[S_LFEND];
    return RV_OK;
}
#undef CDCHK
#undef CDNEED

}  // namespace rv
