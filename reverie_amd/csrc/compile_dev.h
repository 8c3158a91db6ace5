// Gate-stream compiler on the GPU (compile_dev.hip): the compile of a whole GF(2) program, from an op list in device memory, to a
// Compiled identical field by field to what compile_ops makes of it.  Two forms: K = 1 (force_lazy_k = 0; every Xor of two rows
// materialised), when that is a compile compile_ops_seq would keep (lazy_forms_pay false), and the lazy-sum form (force_lazy_k =
// RV_LIN_K, what RV_COMPILE_WHOLE_PROVER asks for: sums of up to RV_LIN_K rows stay symbolic by Builder::g_xor's rule at lazy_slack 1,
// balance 0), which is final for every circuit.  Scope: GF(2) ops only (no Z64, B2A or SizeHint), RV_COMPILE_KEEP_WIRES only under the
// fourth bit below, no other forced lazy_k, no RV_LAZY_K in the environment, at most 2^16 topological rounds.  Everything else, every
// op-list error included, is RV_COMPILE_FALLBACK: the caller runs compile_ops, which returns the canonical result or error code.
//
// RV_COMPILE_DEVICE_Z64 in device_bits: the list may also hold Z64 ops (all ten opcodes) and SizeHint ops that grow neither wire count.
// The GF(2) ops of such a list go through the same pipeline, in either form; every Z64 op becomes one Gate64 at one level above its
// deepest operand, and the two domains share the level numbering (the deeper one's count; the other's tables have empty trailing
// levels).  Still RV_COMPILE_FALLBACK: a B2A op, a SizeHint that grows a wire count, RV_COMPILE_KEEP_WIRES without its bit, RV_LAZY_K, an op-list
// error in either domain, more than 2^16 rounds in either domain, and a plain whole-program compile for which lazy_forms_pay holds.
//
// RV_COMPILE_DEVICE_B2A in device_bits (with RV_COMPILE_DEVICE_Z64 only): the list may also hold B2A ops, whole or as a chunk, in either form.  Where
// the list is split by domain a B2A contributes its 442 SSA-producing steps to the GF(2) list as private ops, in Builder::g_* call
// order (run_pass, case RV_DOM_B2A: 64 Random, Mul and Xor, 62 x {Xor, Xor, Mul, Xor, Xor}, two Xor, 64 reconstructions), and one op
// to the Z64 list.  The private ops write no wire; their operands inside the expansion are fixed places, and only the 64 reads of
// the source wires go through the last-writer search.  A reconstruction is an AssertZero with a value: a computed row of its own,
// counted in n_random_or_recon and absent from the AssertZero tables.  The Gate64 sits one level above its deepest reconstruction:
// the Z64 ops' levels are made once the GF(2) ops have theirs.  RV_COMPILE_FALLBACK, each the host compiler's to compile or report:
//   - RV_COMPILE_KEEP_WIRES without RV_COMPILE_DEVICE_KEEP_WIRES (the wire tables are built under that bit only);
//   - a SizeHint that grows a wire count (the wire tables are sized once);
//   - RV_LAZY_K in the environment, or any forced lazy_k other than RV_LIN_K (forms the device does not build);
//   - any op-list error, a B2A's among them: dst >= z64_wires, src + 64 > gf2_wires (also when src + 64 wraps), reserved != 0;
//   - more than 2^16 rounds in either domain (one adder takes about 190);
//   - a plain whole-program compile for which lazy_forms_pay holds -- B2A programs are deep, so of them only wide ones (some 100
//     adders side by side) are final at K = 1; the lazy-sum form takes them all;
//   - an expanded GF(2) list of 2^28 entries or more.
//
// RV_COMPILE_DEVICE_KEEP_WIRES in device_bits: `keep_wires` (RV_COMPILE_KEEP_WIRES, whole programs only) is no fallback, in any of the
// scopes above and in both forms; every other fallback rule stands.  The result is compile_ops(..., keep_wires = true)'s, wire_forms
// and wire_ssa64 included, in three more steps on the compile's stream:
//   - liveness (before the values): one more read of every written GF(2) wire's last writer, the one the chunk mode's write-back
//     search finds -- per wire, not per distinct value; reads are still counted, so an unread sum that is no wire's final value is
//     dropped as before, and in the lazy rule the extra read is part of f;
//   - wire forms (after the rows have their numbers): one thread per GF(2) wire, the last writer's value with its rows numbered as a
//     gate's operands are, unused slots the zero row, a never-written wire the all-zero form;
//   - Z64: wire w's final SSA id from the Z64 list's writers sort (0: never written; a B2A's Gate64 counts like any writer).
// Both tables stay in device memory for the circuit (DevCompileKeep) and are downloaded into `out` with the rest.
//
// Chunk mode (`chunk` not null): one piece of a stream, identical to compile_ops_seq(..., chunk) -- the wires start in their carried
// rows, the counters at the ChunkStart's, no sum is dropped as unread, and one more level writes every wire the piece wrote back to
// its carried row.  A chunk is final at K = 1 whatever its shape (lazy_forms_pay does not apply; a forced lazy_k is a fallback); an
// empty piece is compiled too.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "compile.h"

namespace rv {

// device memory of the compile: taken and given back through the caller's allocator (the context arena)
struct DevAlloc {
    void* self = nullptr;
    int (*alloc)(void* self, size_t bytes, void** out) = nullptr;  // RV_OK or RV_E_NOMEM
    void (*release)(void* self, void* p) = nullptr;
};

// per-phase times of the last device compile (HIP events on the compile's stream, ms)
struct DevCompileLaps {
    float classify = 0, writers = 0, levels = 0, tables = 0, download = 0;
    uint32_t rounds = 0;  // topological rounds launched
    float z64 = 0;        // RV_COMPILE_DEVICE_Z64, a list with Z64 ops: the split and the Z64 ops' steps (the five above are then the GF(2) ops')
};

// The device arrays a device compile leaves for the circuit (null: freed before the call returns, nothing is kept)
struct DevCompileKeep {
    Gate* d_gates = nullptr;
    uint32_t* d_rec_rows = nullptr;
    uint32_t* d_in_rows = nullptr;
    // a list with Z64 ops (RV_COMPILE_DEVICE_Z64; null otherwise)
    Gate64* d_gates64 = nullptr;
    uint64_t* d_rec_offs64 = nullptr;
    uint64_t* d_in_offs64 = nullptr;
    // keep_wires under RV_COMPILE_DEVICE_KEEP_WIRES: Compiled::wire_forms / wire_ssa64 (null: no wire of that domain)
    WireForm* d_wire_forms = nullptr;
    uint32_t* d_wire_ssa64 = nullptr;
};

// the three bits that choose the compiler: RV_COMPILE_DEVICE_Z64 widens RV_COMPILE_DEVICE's scope and means nothing without it,
// RV_COMPILE_DEVICE_B2A widens RV_COMPILE_DEVICE_Z64's in the same way
constexpr uint32_t RV_COMPILE_DEVICE_BITS = RV_COMPILE_DEVICE | RV_COMPILE_DEVICE_Z64 | RV_COMPILE_DEVICE_B2A;
// (RV_COMPILE_DEVICE_KEEP_WIRES is not among them: it belongs to whole-program compiles, and the contexts' and streams' flag setters
// answer "unknown flag bits" for it)

struct DevCompileRequest {
    const rv_op* d_ops = nullptr;  // n_ops packed rv_op records in device memory (read only)
    size_t n_ops = 0;
    size_t z64_wires = 0, gf2_wires = 0;
    bool keep_wires = false;  // a fallback unless device_bits has RV_COMPILE_DEVICE_KEEP_WIRES
    int force_lazy_k = 0;
    const ChunkStart* chunk = nullptr;
    uint32_t device_bits = 0;  // the caller's compile flags & (RV_COMPILE_DEVICE_BITS | RV_COMPILE_DEVICE_KEEP_WIRES)
};

// RV_OK (out filled; compile_us / upload_us / device_bytes / scratch_bytes left zero), RV_COMPILE_FALLBACK, or RV_E_NOMEM /
// RV_E_DEVICE.  Runs on `st`; synchronises it before returning.
int compile_ops_device(hipStream_t st, const DevAlloc& A, const DevCompileRequest& req, Compiled& out, DevCompileKeep* keep,
                       DevCompileLaps* laps = nullptr);

}  // namespace rv
