// see compile_dev.h
//
// One translation unit: compile_dev_prims.inc (scan, radix sort, Scratch, the error macros, the lap timer), compile_dev_gf2.inc (the GF(2)
// pipeline: the k_cd_* kernels, the value rules, gf2_levels, gf2_tables), compile_dev_z64.inc (a mixed list's split and Z64 ops: the k_z_*
// kernels, z64_split, z64_levels, z64_tables) and this file (build_dag, the one host step both domains share; the drivers).
//
// A whole GF(2) program at K = 1 (every XOR of two distinct rows materialised) or in the lazy-sum form (value_lazy and the LAZY
// instantiations of steps 3 and 5), in the steps of the host compiler (compile.cpp: run_pass, Builder, the (level, class) sort and the
// pipelining tables); each step's kernels say the rest:
//   1. classify   one thread per op: validation (any error -> the flag word -> the host compiler), the counters Builder::g_* keep
//                 (masks, Mul, AssertZero, Input: one exclusive scan gives every gate's m / eo / ep / x), the ordinal tables
//   2. writers    build_dag: the writes sorted by wire, every read's last writer (none: the never-written wire, SSA 0), every value's
//                 reads (pass 1's `uses`) and each op's pending operands
//   3. levels     Kahn rounds over the op DAG, one bounded launch per round; a value and its level by the rules of Builder::g_*
//   4. rows       computed rows numbered in program order after the zero row (a scan of the materialised XORs)
//   5. tables     (level, class) keys, a stable radix sort of the gates, the records written straight into the circuit's gate array,
//                 the LevelRange bounds, the per-level mask-block maxima and the online rows' levels (-> level_done_on)
// gf2_levels is steps 1 - 3, gf2_tables the rest.  No kernel waits for another workgroup; every loop is bounded by the op count, the
// level count or a round cap.
//
// Chunk mode (a ChunkStart: one piece of a stream, compile_ops_seq's `chunk`): a read with no write before it in the piece resolves to
// the wire's carried row (producer -2 - wire instead of -1), the counters start at the ChunkStart's, nothing is dropped as unread, and
//   6. write-back  a flag scan over the wires (written; final form still reads a carried row) numbers the extra computed rows and the
//                  gates of the write-back level, which go straight to their places: the materialised carried forms are level 0's
//                  class 3, the write-backs the last level's, both in wire order -- no op gate has class 3 at K = 1
//
// RV_COMPILE_KEEP_WIRES (RV_COMPILE_DEVICE_KEEP_WIRES; whole programs): between steps 2 and 3 every written wire's last writer gets one
// more read (k_cd_live: the final values are live out of the program), after step 5 the wires' final forms are written from the last
// writers' values (k_cd_wire_forms), and the Z64 wires' final SSA ids come from the Z64 list's writers sort (k_z_wire_ssa).
//
// Z64 ops and mixed lists (RV_COMPILE_DEVICE_Z64).  The two domains share no wire and, without B2A, no gate: run_pass keeps them apart
// except for the level count.  So a mixed list is split (z64_split): its GF(2) ops, compacted in order, go through the pipeline above
// unchanged, and its Z64 ops through the same steps in a simpler form (z64_levels, z64_tables) -- no folding, every op one Gate64, every
// counter a prefix sum, a gate's level one above its deepest operand.  B2A (RV_COMPILE_DEVICE_B2A) is the one dependency between
// them, and it runs one way: a B2A is expanded at the split into its 442 GF(2) steps (k_z_expand) and one Z64-list record.  Hence
// compile_mixed's order: z64_split, gf2_levels, z64_levels (a B2A record's level comes from its reconstructions', k_z_b2a_levels),
// gf2_tables (the level count is the deeper domain's; it fills every B2A's rows), z64_tables (which reads those rows).
#include "compile_dev.h"

#include <stdlib.h>
#include <algorithm>
#include <vector>

namespace rv {
namespace {
#include "compile_dev_prims.inc"

// Step 2 of either domain, the op DAG of one list.  sk / sv: the writes sorted by wire (keys: a wire, W for an op that writes none;
// values: op indices), left in place for the write-back steps -- the pair (kbuf[which], vbuf[which]) of build_dag's buffers; prod: every
// operand's producer; uses, cons_off, cons: each op's consumers (CSR); rem: its pending operands; frontier, rounds: round 0, seeded
struct Dag {
    int which;
    uint32_t *sk, *sv, *seg_lo, *seg_hi, *uses, *rem, *cons_off, *cons, *frontier, max_rounds;
    int2* prod;
    uint2* rounds;
};
int build_dag(Scratch& S, hipStream_t st, const rv_op* ops, size_t n, uint32_t W, uint32_t chunk, uint32_t* kbuf[2], uint32_t* vbuf[2], Dag& D);

#include "compile_dev_gf2.inc"
#include "compile_dev_z64.inc"

// (kbuf[0], vbuf[0]): the sort keys and op indices, filled by the caller (k_cd_classify, k_z_wkeys).  RV_OK, RV_E_NOMEM or RV_E_DEVICE.
int build_dag(Scratch& S, hipStream_t st, const rv_op* ops, size_t n, uint32_t W, uint32_t chunk, uint32_t* kbuf[2], uint32_t* vbuf[2], Dag& D) {
    const uint32_t gb = blocks(n, TB);
    CDCHK(radix_sort(S, st, kbuf, vbuf, n, bit_len(W), &D.which));
    D.sk = kbuf[D.which], D.sv = vbuf[D.which];
    D.seg_lo = S.get<uint32_t>(W);
    D.seg_hi = S.get<uint32_t>(W);
    D.prod = S.get<int2>(n);
    D.uses = S.get<uint32_t>(n + 1);
    D.rem = S.get<uint32_t>(n);
    CDNEED(D.seg_lo && D.seg_hi && D.prod && D.uses && D.rem);
    CDCHK(hipMemsetAsync(D.seg_lo, 0, std::max<size_t>(W, 1) * 4, st));
    CDCHK(hipMemsetAsync(D.seg_hi, 0, std::max<size_t>(W, 1) * 4, st));
    CDCHK(hipMemsetAsync(D.uses, 0, (n + 1) * 4, st));
    k_cd_segs<<<gb, TB, 0, st>>>(D.sk, n, W, D.seg_lo, D.seg_hi);
    k_cd_resolve<<<gb, TB, 0, st>>>(ops, n, D.sv, D.seg_lo, D.seg_hi, chunk, D.prod, D.uses, D.rem);
    CDCHK(hipGetLastError());
    D.cons_off = S.get<uint32_t>(n + 1);
    uint32_t* cursor = S.get<uint32_t>(n);
    D.cons = S.get<uint32_t>(2 * n);
    CDNEED(D.cons_off && cursor && D.cons);
    CDCHK((scan_excl<uint32_t, SumU32>(S, st, D.uses, D.cons_off, n + 1, nullptr)));
    CDCHK(hipMemsetAsync(cursor, 0, n * 4, st));
    k_cd_consumers<<<gb, TB, 0, st>>>(D.prod, n, D.cons_off, cursor, D.cons);
    CDCHK(hipGetLastError());
    D.frontier = S.get<uint32_t>(n);
    D.max_rounds = (uint32_t)std::min<size_t>(n + 1, MAX_ROUNDS);
    D.rounds = S.get<uint2>((size_t)D.max_rounds + 2);
    CDNEED(D.frontier && D.rounds);
    CDCHK(hipMemsetAsync(D.rounds, 0, ((size_t)D.max_rounds + 2) * sizeof(uint2), st));
    k_cd_front0<<<gb, TB, 0, st>>>(D.rem, n, D.frontier, D.rounds);
    CDCHK(hipGetLastError());
    return RV_OK;
}

// DevCompileLaps from the marks, after the last stream sync (z64: the list had Z64 entries -- the GF(2) levels lap is the two stretches around theirs)
void fill_laps(const LapTimer& T, uint32_t rounds, bool z64, DevCompileLaps& laps) {
    laps.classify = T.ms(LAP_BEGIN, LAP_CLASSIFIED), laps.writers = T.ms(LAP_CLASSIFIED, LAP_DAG);
    laps.levels = z64 ? T.ms(LAP_DAG, LAP_Z64_LEVELS) + T.ms(LAP_Z64_LEVELS_END, LAP_LEVELS) : T.ms(LAP_DAG, LAP_LEVELS);
    laps.tables = T.ms(LAP_LEVELS, LAP_TABLES), laps.download = T.ms(LAP_TABLES, LAP_DOWNLOADED);
    laps.rounds = rounds;
    if (z64) laps.z64 = T.ms(LAP_SPLIT, LAP_SPLIT_END) + T.ms(LAP_Z64_LEVELS, LAP_Z64_LEVELS_END) + T.ms(LAP_Z64_TABLES, LAP_Z64_TABLES_END);
}

// a GF(2) list: the caller's own.  R (both drivers): the result Scratch, or null when the caller keeps nothing -- a phase's result
// arrays then come from its work Scratch and go back with it.
int compile_gf2(hipStream_t st, const DevAlloc& A, const DevCompileRequest& q, Scratch* R, LapTimer& T, Compiled& out, DevCompileKeep& res,
                DevCompileLaps* laps) {
    Gf2State g{};
    g.ops = q.d_ops, g.n = q.n_ops;
    if (const int rc = gf2_begin(q, g)) return rc;
    if (!T.init(LAP_GF2_MARKS)) return RV_E_DEVICE;
    Scratch S(A, st);
    if (const int rc = gf2_levels(S, R ? *R : S, T, st, g)) return rc;
    if (const int rc = gf2_tables(S, R ? *R : S, T, st, g, 0, false, out, &res.d_gates)) return rc;
    res.d_rec_rows = g.rec_rows, res.d_in_rows = g.in_rows, res.d_wire_forms = g.wire_forms;
    if (g.keep)  // (a GF(2) list: every Z64 wire reads as SSA 0)
        if (const int rc = z64_wire_table(S, R ? *R : S, st, nullptr, g.z64_wires, out, &res.d_wire_ssa64)) return rc;
    if (laps) fill_laps(T, g.rounds, false, *laps);
    return RV_OK;
}

// a list that may hold Z64, SizeHint and (RV_COMPILE_DEVICE_B2A in device_bits) B2A ops
int compile_mixed(hipStream_t st, const DevAlloc& A, const DevCompileRequest& q, Scratch* R, LapTimer& T, Compiled& out, DevCompileKeep& res,
                  DevCompileLaps* laps) {
    const size_t n = q.n_ops;
    const ChunkStart* chunk = q.chunk;
    const bool lazy = q.force_lazy_k == RV_LIN_K;
    const bool keep_here = (q.device_bits & RV_COMPILE_DEVICE_KEEP_WIRES) && !chunk;  // (the wires' final values: whole programs, under their bit)
    if ((q.keep_wires && !keep_here) || (q.force_lazy_k && (!lazy || chunk)) || getenv("RV_LAZY_K") || n >= (1u << 28) || q.gf2_wires >= (1u << 31) ||
        q.z64_wires >= (1u << 30))
        return RV_COMPILE_FALLBACK;
    if (n == 0) return compile_gf2(st, A, q, R, T, out, res, laps);  // (an empty piece; an empty program is the host compiler's)
    if (chunk && (chunk->mask64_phase >= 2 || chunk->on_words64_0 > (1ull << 62) || chunk->pre_words64_0 > (1ull << 62))) return RV_COMPILE_FALLBACK;
    if (!T.init(LAP_MARKS)) return RV_E_DEVICE;
    Scratch S(A, st);  // the split and the Z64 steps
    Z64State z{};
    if (const int rc = z64_split(S, T, st, q, z)) return rc;
    if (z.no_z64()) return compile_gf2(st, A, q, R, T, out, res, laps);
    const Mixed mx{z.orig2, n, z.n_b2a, z.b2a_base, z.b2a_rows};
    Gf2State g{};
    g.ops = z.ops2, g.n = z.n2, g.mx = &mx;
    if (const int rc = gf2_begin(q, g)) return rc;
    {
        Scratch S2(A, st);  // the GF(2) steps: given back before the Z64 tables are allocated
        if (const int rc = gf2_levels(S2, R ? *R : S2, T, st, g)) return rc;
        if (const int rc = z64_levels(S, T, st, z, g.glvl)) return rc;
        if (const int rc = gf2_tables(S2, R ? *R : S2, T, st, g, z.levels64, z.n_wb64 != 0, out, &res.d_gates)) return rc;
        res.d_rec_rows = g.rec_rows, res.d_in_rows = g.in_rows, res.d_wire_forms = g.wire_forms;
    }
    if (const int rc = z64_tables(S, R ? *R : S, T, st, z, g.keep, out, res)) return rc;
    if (laps) fill_laps(T, g.rounds, z.n64 != 0, *laps);
    return RV_OK;
}
}  // namespace

int compile_ops_device(hipStream_t st, const DevAlloc& A, const DevCompileRequest& q, Compiled& out, DevCompileKeep* keep, DevCompileLaps* laps) {
    if (keep) *keep = DevCompileKeep();
    const bool mixed = (q.device_bits & RV_COMPILE_DEVICE_Z64) != 0;
    LapTimer T(st, laps != nullptr);
    // The result Scratch: the arrays a circuit may keep (DevCompileKeep), handed over in one place, after a successful compile (a failure frees all through
    // the destructors).  Declared first, so it is released after every work Scratch, whose destructor synchronised the stream.
    Scratch R(A, st, false);
    DevCompileKeep res;
    const int rc = mixed ? compile_mixed(st, A, q, keep ? &R : nullptr, T, out, res, laps) : compile_gf2(st, A, q, keep ? &R : nullptr, T, out, res, laps);
    if (rc == RV_OK && keep) *keep = res, R.keep_all();  // (R holds these arrays and nothing else)
    return rc;
}
#undef CDCHK
#undef CDNEED

}  // namespace rv
