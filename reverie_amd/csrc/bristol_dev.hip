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
// Work memory: 8 bytes per gate line the header names (n_gates <= len / 8 + 1: the text, not the header, bounds it), 8 bytes per tile
// and the scans' sums.
#include "bristol_dev.h"

#include <algorithm>
#include <vector>

namespace rv {
namespace {
#include "compile_dev_prims.inc"
[[maybe_unused]] const auto unused_sort = &radix_sort;  // (the scans are all this file takes from the building blocks)
static_assert(TB * 16 == BRISTOL_TILE_BYTES, "a lane takes 16 bytes of a tile");
static_assert(TB == BRISTOL_WG_LINES, "a thread per line");

// the words of one call in device memory (64-bit each)
enum { S_ERR, S_LINES, S_OPS, S_AND, S_XOR, S_INV, S_OTHER, S_WORDS };
constexpr uint64_t NO_ERR = ~0ull;

// ---- steps 1 and 2 ----
// the 16 bytes at c that lie in [lo, hi): bit k of lf / tok = byte k is a line feed / a token byte
__device__ inline void classify16(const uint8_t* c, const uint8_t* lo, const uint8_t* hi, uint32_t& lf, uint32_t& tok) {
    lf = tok = 0;
    if (c >= hi || c + 16 <= lo) return;
    if (c >= lo && c + 16 <= hi) {  // (c is 16-byte aligned: the tiles start at an aligned address)
        const uint4 v = *reinterpret_cast<const uint4*>(c);
        const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int k = 0; k < 16; k++) {
            const uint32_t b = (w[k >> 2] >> (8 * (k & 3))) & 255u;
            if (b == '\n') lf |= 1u << k;
            else if (b != ' ' && b != '\t' && b != '\r') tok |= 1u << k;
        }
    } else {
        for (int k = 0; k < 16; k++) {
            if (c + k < lo || c + k >= hi) continue;
            const uint32_t b = c[k];
            if (b == '\n') lf |= 1u << k;
            else if (b != ' ' && b != '\t' && b != '\r') tok |= 1u << k;
        }
    }
}
// LINES false: tkey[t] = the tile's scan key, tmeta[t] = its line count had it begun at a line's start | bit 31: the first of them is
// no line start when the tile begins inside a line with a token.  LINES true: tin = the keys' exclusive max-scan, tbase = the first
// line index of every tile; the line table.
template <bool LINES>
__global__ __launch_bounds__(TB) void k_bp_tiles(const uint8_t* text, const uint8_t* base, const uint8_t* lo, const uint8_t* hi, uint32_t* tkey,
                                                 uint32_t* tmeta, const uint32_t* tin, const uint32_t* tbase, uint64_t n_gates, uint32_t* line_off) {
    __shared__ uint32_t sh[TB];
    __shared__ uint32_t cond;
    if (threadIdx.x == 0) cond = 0;
    const uint8_t* c = base + (size_t)blockIdx.x * BRISTOL_TILE_BYTES + (size_t)threadIdx.x * 16;
    uint32_t lf, tok;
    classify16(c, lo, hi, lf, tok);
    // the state a lane begins in: the flag of the last lane before it that holds anything but whitespace, else the tile's
    const uint32_t after = lf ? tok >> (32 - __clz(lf)) : tok;  // token bytes behind the lane's last LF
    const uint32_t key = (lf | tok) ? ((threadIdx.x + 1u) << 1 | (after ? 1u : 0u)) : 0u;
    uint32_t last;
    const uint32_t prev = block_excl<uint32_t, MaxU32>(key, sh, &last);
    const uint32_t tile_in = LINES ? (tin[blockIdx.x] & 1u) : 0u;
    uint32_t s = prev ? (prev & 1u) : tile_in;
    uint32_t starts = 0;  // bit k: a gate line's first token byte
    for (int k = 0; k < 16; k++) {
        if ((lf >> k) & 1u) s = 0;
        else if ((tok >> k) & 1u) {
            if (!s) starts |= 1u << k;
            s = 1;
        }
    }
    if (!LINES && !prev && (lf | tok)) cond = tok && (!lf || __ffs(tok) < __ffs(lf));  // (one lane at most: the first with content)
    uint32_t total;
    const uint32_t ex = block_excl<uint32_t, SumU32>(__popc(starts), sh, &total);
    if (!LINES) {
        if (threadIdx.x == 0) {
            tkey[blockIdx.x] = last ? ((blockIdx.x + 1u) << 1 | (last & 1u)) : 0u;
            tmeta[blockIdx.x] = total | (cond << 31);
        }
    } else {
        uint64_t idx = (uint64_t)tbase[blockIdx.x] + ex;
        for (int k = 0; k < 16 && idx < n_gates; k++)
            if ((starts >> k) & 1u) line_off[idx++] = (uint32_t)(c + k - text);
    }
}
__global__ __launch_bounds__(TB) void k_bp_counts(const uint32_t* tin, uint32_t* tmeta, uint32_t n_tiles) {
    const uint32_t t = blockIdx.x * TB + threadIdx.x;
    if (t >= n_tiles) return;
    const uint32_t m = tmeta[t];
    tmeta[t] = (m & 0x7FFFFFFFu) - ((m >> 31) & tin[t] & 1u);
}

// ---- steps 3 and 4 ----
// a cursor over one line's tokens
struct Cur {
    const uint8_t* p;
    const uint8_t* hi;
    // the next token, false at the line's end.  v: its value by the host's rule (to_u64 of bristol.cpp); st: 0 for a number below 2^32,
    // RV_E_BAD_OP when not all digits, RV_E_UNSUPPORTED when all digits and 2^32 or more; head: its first four bytes, n: its length
    __device__ bool next(uint64_t& v, int& st, uint32_t& head, uint32_t& n) {
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
    __device__ bool next(uint64_t& v) {
        int st;
        uint32_t head, n;
        return next(v, st, head, n);
    }
};
constexpr uint32_t kind3(char a, char b, char c) { return (uint32_t)a | (uint32_t)b << 8 | (uint32_t)c << 16; }
enum { K_NONE, K_XOR, K_AND, K_INV, K_EQW, K_EQ, K_MAND };
__device__ inline int kind_of(uint32_t head, uint32_t n) {  // (case-sensitive, as the host's string compares)
    if (n == 3) {
        if (head == kind3('X', 'O', 'R')) return K_XOR;
        if (head == kind3('A', 'N', 'D')) return K_AND;
        if (head == kind3('I', 'N', 'V') || head == kind3('N', 'O', 'T')) return K_INV;
        if (head == kind3('E', 'Q', 'W')) return K_EQW;
    }
    if (n == 2 && head == ((uint32_t)'E' | (uint32_t)'Q' << 8)) return K_EQ;
    if (n == 4 && head == (kind3('M', 'A', 'N') | (uint32_t)'D' << 24)) return K_MAND;
    return K_NONE;
}

__global__ __launch_bounds__(TB) void k_bp_validate(const uint8_t* text, const uint8_t* hi, const uint32_t* line_off, uint64_t n_gates,
                                                    uint64_t n_wires, uint32_t* cnt, uint64_t* state) {
    __shared__ unsigned long long cls[4];  // and, xor, inv, other
    if (threadIdx.x < 4) cls[threadIdx.x] = 0;
    __syncthreads();
    const uint64_t i = (uint64_t)blockIdx.x * TB + threadIdx.x;
    const uint64_t found = state[S_LINES];
    int code = 0, cl = -1;
    uint64_t recs = 0;
    if (i < n_gates && i >= found) {
        if (i == found) code = RV_E_BAD_OP;  // the file is short: the host fails at the first line it cannot read
    } else if (i < n_gates) {
        Cur c{text + line_off[i], hi};
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
        const int kind = kind_of(head, n);
        if (ntok < 4) code = RV_E_BAD_OP;
        else if (numerr) code = numerr;
        else if (ntok - 1 != 2 + nin + nout) code = RV_E_BAD_OP;
        else if (kind == K_XOR || kind == K_AND) {
            if (nin != 2 || nout != 1) code = RV_E_BAD_OP;
            else if (oob) code = RV_E_WIRE_OOB;
            cl = kind == K_AND ? 0 : 1, recs = 1;
        } else if (kind == K_INV || kind == K_EQW) {
            if (nin != 1 || nout != 1) code = RV_E_BAD_OP;
            else if (oob) code = RV_E_WIRE_OOB;
            cl = kind == K_INV ? 2 : 3, recs = 1;
        } else if (kind == K_EQ) {  // the "input" is the literal
            if (nin != 1 || nout != 1 || v2 > 1) code = RV_E_BAD_OP;
            else if (v3 >= n_wires) code = RV_E_WIRE_OOB;
            cl = 3, recs = 1;
        } else if (kind == K_MAND) {
            if (nin != 2 * nout || nout == 0) code = RV_E_BAD_OP;
            else if (oob) code = RV_E_WIRE_OOB;
            cl = 0, recs = nout;
        } else {
            code = RV_E_BAD_OP;
        }
    }
    if (i < n_gates) cnt[i] = code ? 0u : (uint32_t)recs;
    if (code) atomicMin((unsigned long long*)&state[S_ERR], (unsigned long long)(i << 8 | (uint64_t)code));
    else if (cl >= 0) atomicAdd(&cls[cl], (unsigned long long)recs);
    __syncthreads();
    if (threadIdx.x < 4 && cls[threadIdx.x]) atomicAdd((unsigned long long*)&state[S_AND + threadIdx.x], cls[threadIdx.x]);
}

__device__ inline void put(uint64_t* out, uint64_t at, uint32_t opcode, uint32_t dst, uint32_t a, uint32_t b, uint64_t imm) {
    uint64_t* r = out + at * 3;  // rv_op: domain (GF(2): 0), opcode, reserved, dst | a, b | imm
    r[0] = (uint64_t)opcode << 8 | (uint64_t)dst << 32;
    r[1] = (uint64_t)a | (uint64_t)b << 32;
    r[2] = imm;
}
// the records are written when the text has no error and they fit (fixed: the inputs and the assertion records)
__device__ inline bool emit_wanted(const uint64_t* state, uint64_t fixed, uint64_t cap) {
    return state[S_ERR] == NO_ERR && state[S_OPS] + fixed <= cap;
}
__global__ __launch_bounds__(TB) void k_bp_emit(const uint8_t* text, const uint8_t* hi, const uint32_t* line_off, const uint32_t* first, uint64_t n_gates,
                                                const uint64_t* state, uint64_t fixed, uint64_t cap, uint64_t n_inputs, uint64_t* out) {
    if (!emit_wanted(state, fixed, cap)) return;
    const uint64_t i = (uint64_t)blockIdx.x * TB + threadIdx.x;
    if (i >= n_gates) return;
    const Cur start{text + line_off[i], hi};
    Cur c = start;
    uint64_t v = 0, w[5] = {0, 0, 0, 0, 0}, ntok = 0;
    int st;
    uint32_t head = 0, n = 0;
    while (c.next(v, st, head, n)) {
        if (ntok < 5) w[ntok] = v;
        ntok++;
    }
    const uint64_t at = n_inputs + first[i];
    switch (kind_of(head, n)) {
    case K_XOR: put(out, at, RV_OP_ADD, (uint32_t)w[4], (uint32_t)w[2], (uint32_t)w[3], 0); break;
    case K_AND: put(out, at, RV_OP_MUL, (uint32_t)w[4], (uint32_t)w[2], (uint32_t)w[3], 0); break;
    case K_INV: put(out, at, RV_OP_ADDCONST, (uint32_t)w[3], (uint32_t)w[2], 0, 1); break;
    case K_EQW: put(out, at, RV_OP_ADDCONST, (uint32_t)w[3], (uint32_t)w[2], 0, 0); break;
    case K_EQ: put(out, at, RV_OP_CONST, (uint32_t)w[3], 0, 0, w[2]); break;
    case K_MAND: {
        const uint64_t nout = w[1];
        Cur ca = start, cb, co;
        ca.next(v), ca.next(v);
        cb = ca;
        for (uint64_t k = 0; k < nout; k++) cb.next(v);
        co = cb;
        for (uint64_t k = 0; k < nout; k++) co.next(v);
        for (uint64_t k = 0; k < nout; k++) {
            uint64_t a = 0, b = 0, o = 0;
            ca.next(a), cb.next(b), co.next(o);
            put(out, at + k, RV_OP_MUL, (uint32_t)o, (uint32_t)a, (uint32_t)b, 0);
        }
        break;
    }
    default: break;
    }
}
__global__ __launch_bounds__(TB) void k_bp_inputs(const uint64_t* state, uint64_t fixed, uint64_t cap, uint64_t n_inputs, uint64_t* out) {
    if (!emit_wanted(state, fixed, cap)) return;
    for (uint64_t w = (uint64_t)blockIdx.x * TB + threadIdx.x; w < n_inputs; w += (uint64_t)gridDim.x * TB) put(out, w, RV_OP_INPUT, (uint32_t)w, 0, 0, 0);
}
// AddConst(tmp, w, expected) + AssertZero(tmp) for the last n_pairs wires
__global__ __launch_bounds__(TB) void k_bp_asserts(const uint64_t* state, uint64_t fixed, uint64_t cap, uint64_t n_inputs, uint64_t n_wires,
                                                   const uint8_t* expected, uint64_t n_pairs, uint64_t* out) {
    if (!emit_wanted(state, fixed, cap)) return;
    const uint64_t k = (uint64_t)blockIdx.x * TB + threadIdx.x;
    if (k >= n_pairs) return;
    const uint64_t at = n_inputs + state[S_OPS] + 2 * k;
    const uint32_t tmp = (uint32_t)(n_wires + k);
    put(out, at, RV_OP_ADDCONST, tmp, (uint32_t)(n_wires - n_pairs + k), 0, expected[k] & 1u);
    put(out, at + 1, RV_OP_ASSERTZERO, 0, tmp, 0, 0);
}

}  // namespace

int bristol_gates_device(hipStream_t st, const DevAlloc& A, const uint8_t* d_text, size_t len, size_t gates_offset, uint64_t n_gates, uint64_t n_wires,
                         uint64_t n_inputs, const uint8_t* d_expected, uint64_t n_pairs, rv_op* d_ops, uint64_t cap_ops, BristolGates* res) {
    Scratch S(A, st);
    const uint8_t *lo = d_text + gates_offset, *hi = d_text + len;
    const uint8_t* base = lo - ((uintptr_t)lo & 15);  // (bytes before lo are never read: classify16)
    const uint32_t n_tiles = blocks((size_t)(hi - base), BRISTOL_TILE_BYTES);
    uint64_t* state = S.get<uint64_t>(S_WORDS);
    uint32_t *tkey = S.get<uint32_t>(n_tiles), *tmeta = S.get<uint32_t>(n_tiles);
    uint32_t *line_off = S.get<uint32_t>(n_gates), *cnt = S.get<uint32_t>(n_gates);
    CDNEED(state && tkey && tmeta && line_off && cnt);
    const uint32_t gl = blocks(n_gates, TB);

    CDCHK(hipMemsetAsync(state, 0, S_WORDS * 8, st));
    CDCHK(hipMemsetAsync(state, 0xFF, 8, st));
    k_bp_tiles<false><<<n_tiles, TB, 0, st>>>(d_text, base, lo, hi, tkey, tmeta, nullptr, nullptr, n_gates, nullptr);
    CDCHK(hipGetLastError());
    CDCHK((scan_excl<uint32_t, MaxU32>(S, st, tkey, tkey, n_tiles, nullptr)));
    k_bp_counts<<<blocks(n_tiles, TB), TB, 0, st>>>(tkey, tmeta, n_tiles);
    CDCHK((scan_excl<uint32_t, SumU32>(S, st, tmeta, tmeta, n_tiles, (uint32_t*)&state[S_LINES])));
    k_bp_tiles<true><<<n_tiles, TB, 0, st>>>(d_text, base, lo, hi, nullptr, nullptr, tkey, tmeta, n_gates, line_off);
    k_bp_validate<<<gl, TB, 0, st>>>(d_text, hi, line_off, n_gates, n_wires, cnt, state);
    CDCHK(hipGetLastError());
    CDCHK((scan_excl<uint32_t, SumU32>(S, st, cnt, cnt, n_gates, (uint32_t*)&state[S_OPS])));
    const uint64_t fixed = n_inputs + 2 * n_pairs;
    if (d_ops) {
        uint64_t* out = reinterpret_cast<uint64_t*>(d_ops);
        k_bp_emit<<<gl, TB, 0, st>>>(d_text, hi, line_off, cnt, n_gates, state, fixed, cap_ops, n_inputs, out);
        if (n_inputs) k_bp_inputs<<<std::min<uint32_t>(blocks(n_inputs, TB), 1u << 16), TB, 0, st>>>(state, fixed, cap_ops, n_inputs, out);
        if (n_pairs) k_bp_asserts<<<blocks(n_pairs, TB), TB, 0, st>>>(state, fixed, cap_ops, n_inputs, n_wires, d_expected, n_pairs, out);
        CDCHK(hipGetLastError());
    }
    std::vector<uint64_t> h(S_WORDS);
    CDCHK(fetch(st, h, state));
    CDCHK(hipStreamSynchronize(st));
    *res = BristolGates{};
    if (h[S_ERR] != NO_ERR) {
        res->code = (int)(h[S_ERR] & 0xFFu);
        return RV_OK;
    }
    res->gate_ops = h[S_OPS];
    res->n_and = h[S_AND], res->n_xor = h[S_XOR], res->n_inv = h[S_INV], res->n_other = h[S_OTHER];
    res->written = d_ops && h[S_OPS] + fixed <= cap_ops;
    return RV_OK;
}
#undef CDCHK
#undef CDNEED

}  // namespace rv
