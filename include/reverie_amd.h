/* reverie_amd — MI355X-native KKW prover/verifier hot path: C-ABI drop-in boundary.
 *
 * This header is what a Rust `-sys` shim (or any FFI) binds.  It replaces, at the only
 * seam where an FFI call is affordable, the reference's
 *
 *     Proof::new(circuit, wit_gf2, wit_z64, (z64_wires, gf2_wires)) -> Proof
 *                                            /root/reference/src/proof/mod.rs:119-222
 *     Proof::verify(&self, circuit, (z64_wires, gf2_wires)) -> bool
 *                                            /root/reference/src/proof/mod.rs:224-307
 *
 * and everything those two drive: src/generator (AES-CTR share expansion),
 * src/interpreter over src/algebra's packed GF(2)/Z64 rings, src/transcript, and the
 * BLAKE3 commitments / random oracle of src/crypto.  Proof bytes are bincode-1.3
 * compatible with the reference's `Proof`.
 *
 * Plain pointers and sizes only; no C++/torch types.  All functions return RV_OK (0) or
 * an RV_E_* code; nothing aborts the process (the reference panics).
 * A context is bound to ONE GPU and is thread-compatible: one in-flight call per context.
 */
#ifndef REVERIE_AMD_H
#define REVERIE_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---- protocol constants: /root/reference/src/lib.rs:17-38 ---- */
#define RV_PLAYERS 8
#define RV_PACKED 8
#define RV_BATCH_SIZE 128
#define RV_ONLINE_REPS 40
#define RV_TOTAL_REPS 256
#define RV_PREPROCESSING_REPS (RV_TOTAL_REPS - RV_ONLINE_REPS)
#define RV_KEY_SIZE 16  /* src/crypto/prg.rs:9  */
#define RV_HASH_SIZE 32 /* src/crypto/hash.rs:8 */

/* ---- gate stream ------------------------------------------------------------------
 * One record per `mcircuit::CombineOperation` (re-exported at src/lib.rs:7; consumed at
 * src/interpreter/combine.rs:120-132 and src/interpreter/single.rs:106-156).
 *   domain RV_DOM_GF2 / RV_DOM_Z64 : `Operation<bool>` / `Operation<u64>`, opcode below;
 *            fields: Input(dst) Random(dst) Add(dst,a,b) AddConst(dst,a,imm) Sub(dst,a,b)
 *            SubConst(dst,a,imm) Mul(dst,a,b) MulConst(dst,a,imm) AssertZero(a) Const(dst,imm)
 *            (GF2 constants use bit 0 of imm)
 *   domain RV_DOM_B2A      : B2A(dst = z64 wire, a = lowest of 64 consecutive gf2 wires)
 *   domain RV_DOM_SIZEHINT : SizeHint(a = z64 wire count, b = gf2 wire count)
 */
typedef struct rv_op {
    uint8_t domain;
    uint8_t opcode;
    uint16_t reserved; /* must be 0 */
    uint32_t dst;
    uint32_t a;
    uint32_t b;
    uint64_t imm;
} rv_op; /* 24 bytes */

enum { RV_DOM_GF2 = 0, RV_DOM_Z64 = 1, RV_DOM_B2A = 2, RV_DOM_SIZEHINT = 3 };
enum {
    RV_OP_INPUT = 0,
    RV_OP_RANDOM = 1,
    RV_OP_ADD = 2,
    RV_OP_ADDCONST = 3,
    RV_OP_SUB = 4,
    RV_OP_SUBCONST = 5,
    RV_OP_MUL = 6,
    RV_OP_MULCONST = 7,
    RV_OP_ASSERTZERO = 8,
    RV_OP_CONST = 9
};

/* ---- status codes (reference behaviour in parentheses) ---- */
enum {
    RV_OK = 0,
    RV_E_WITNESS_INVALID = 1, /* (panic, src/transcript/prover.rs:221-228) an AssertZero failed */
    RV_E_WITNESS_SHORT = 2,   /* (panic "witness is too short", prover.rs:190) */
    RV_E_WIRE_OOB = 3,        /* (Vec index panic, single.rs:109-155) wire index >= wire count */
    RV_E_PROOF_MALFORMED = 4, /* (bincode unwrap / assert panics; `omit >= 8` is UB upstream) */
    RV_E_BAD_OP = 5,          /* unknown domain/opcode or reserved != 0 */
    RV_E_NOMEM = 6,
    RV_E_DEVICE = 7, /* no usable gfx950 device / HIP runtime error (see rv_last_error) */
    RV_E_UNSUPPORTED = 8,
    RV_E_ARG = 9
};

typedef struct rv_ctx rv_ctx;         /* one GPU: stream, scratch arena                    */
typedef struct rv_circuit rv_circuit; /* a gate stream levelised and resident in HBM       */
typedef struct rv_shard rv_shard;     /* committed repetitions awaiting the challenge      */
typedef struct rv_stream rv_stream;   /* a bounded-memory proof in progress (two passes over a chunked gate stream) */
typedef struct rv_comm rv_comm;       /* this GPU's rank in a group of GPUs proving together (RCCL communicator)   */

const char *rv_strerror(int code);
/* last HIP/driver error text for this thread ("" if none) */
const char *rv_last_error(void);
/* library/ABI version, bumps on any signature change */
uint32_t rv_abi_version(void);

/* ---- context ---- */
int rv_ctx_create(int device_ordinal, rv_ctx **out);
void rv_ctx_destroy(rv_ctx *ctx);
/* A context owns the device memory of the circuits and shards created on it: destroy those first. */
/* block until all work queued on the context's stream has finished */
int rv_ctx_sync(rv_ctx *ctx);

/* ---- per-phase GPU timing, measured with HIP events on the context's own stream (the
 * stream every kernel of this library is launched on).  Phases: */
enum {
    RV_PH_SETUP = 0,  /* seed expansion, key schedules, round-key bitslicing          */
    RV_PH_MASKS = 1,  /* k_aes_gf2_masks: bitsliced AES-128-CTR mask generator         */
    RV_PH_INTERP = 2, /* k_interp_full / k_interp64: one launch per dependency level; k_interp_lds (or k_interp_narrow): one per narrow stretch */
    RV_PH_HASH = 3,   /* k_b3_chunks(_bits,_contig) + k_b3_reduce + k_b3_tree_tail: transcript BLAKE3 */
    RV_PH_JOIN = 4,   /* k_join                                                        */
    RV_PH_OPEN = 5,   /* k_fs_challenge + k_open_headers + k_extract_rows / k_extract_from_bits / k_extract64 */
    RV_PH_EARLY = 6,  /* launches only (their time is inside RV_PH_INTERP): k_pack_corr_all + k_publish of rv_prove's early-corrections path */
    RV_PH_CLEAR = 7,  /* unused since round 6 (the flat prover schedule's cleartext pass): the slot stays so that rv_profile keeps its size */
    RV_PH_COUNT = 8
};
typedef struct rv_profile {
    double ms[RV_PH_COUNT];         /* accumulated GPU milliseconds per phase */
    uint64_t launches[RV_PH_COUNT]; /* kernel launches per phase              */
    uint64_t calls;                 /* commit / verify_shard calls accumulated */
} rv_profile;
/* enable != 0 turns event timing on (a stream event per phase boundary: every one costs the call ~5 us of idle GPU; enable == 2: only
 * the interpreter's phase, RV_PH_INTERP, is timed -- two events per call); reset != 0 zeroes the accumulators; out (nullable) receives
 * the current totals. */
int rv_ctx_profile(rv_ctx *ctx, int enable, int reset, rv_profile *out);

/* ---- circuit: the `Arc<Vec<CombineOperation>>` + `wire_counts` arguments of
 * Proof::new / Proof::verify (proof/mod.rs:119-125,224,232).  Compiling resolves wire
 * reuse, orders gates into dependency levels, assigns every gate its PRG mask index and
 * transcript offsets, and uploads the result to HBM; it is reusable across proofs.
 * Errors that the reference raises while stepping (wire out of range, bad op) are
 * reported here. */
int rv_circuit_compile(rv_ctx *ctx, const rv_op *ops, size_t n_ops, size_t z64_wires, size_t gf2_wires,
                       rv_circuit **out);
/* The same with a hint about how the circuit will be used.  Every entry point accepts any compiled circuit and
 * produces identical bytes; the hint only chooses between gate streams that different users run at different speeds.
 * RV_COMPILE_WHOLE_PROVER: mostly proofs of all 256 repetitions on one GPU (rv_prove, rv_prove_device,
 * rv_prove_batch -- what Proof::new does, proof/mod.rs:119-175).  Linear gates of wide circuits are then kept as
 * lazy sums of up to three rows instead of being materialised: the whole-proof interpreter keeps one cleartext value
 * byte per row and reads full 256-byte rows, so the extra operand rows cost less than the Xor gates they replace (10^7-gate
 * benchmark circuit: rv_prove 6.4 -> 6.15 ms); the verifier and repetition shards (32-byte to 128-byte rows, corr-bit
 * rows per operand) run 3-15 % slower on such a stream, so rv_circuit_compile does not choose it. */
#define RV_COMPILE_WHOLE_PROVER 1u
/* RV_COMPILE_KEEP_WIRES: the circuit also keeps, in HBM, the value form every wire has at the end of the program (GF(2): at most
 * three share rows plus a constant bit; Z64: the final SSA id; a wire that is never written reads as zero) -- what rv_evaluate needs
 * to return wire values.  Proofs of such a circuit are byte-identical to those of a circuit compiled without it. */
#define RV_COMPILE_KEEP_WIRES 2u
int rv_circuit_compile_ex(rv_ctx *ctx, const rv_op *ops, size_t n_ops, size_t z64_wires, size_t gf2_wires, uint32_t flags,
                          rv_circuit **out);
/* RV_COMPILE_DEVICE: the op list is uploaded and compiled on the context's GPU (csrc/compile_dev.hip) into a circuit identical field
 * by field to the host compiler's, so every proof, verification and evaluation is byte-identical.  The device path takes whole
 * programs of GF(2) ops (no Z64, B2A or SizeHint op) in either gate-stream form: the plain one (every Xor of two rows materialised)
 * when that is the host compiler's final answer -- not for the deep, narrow circuits it recompiles with lazy sums (AES-128, SHA-256)
 * --, and, combined with RV_COMPILE_WHOLE_PROVER, the lazy-sum form of any such program (a forced form is final, so AES-128 and
 * SHA-256 compile on the device under both flags).  Not with RV_COMPILE_KEEP_WIRES (unless RV_COMPILE_DEVICE_KEEP_WIRES is set as
 * well, below) or RV_LAZY_K, and not past 2^16 dependency
 * rounds.  Everything else, op-list errors included, is compiled by the host compiler, with its error codes;
 * rv_circuit_compiled_on_device tells which compiler made a circuit. */
#define RV_COMPILE_DEVICE 4u
/* RV_COMPILE_DEVICE_Z64, only together with RV_COMPILE_DEVICE (on its own it is RV_E_ARG; rv_circuit_compile_device implies
 * RV_COMPILE_DEVICE, so it may be passed to that call alone): the device compiler also takes Z64 ops -- all ten opcodes -- and
 * SizeHint ops that grow neither wire count, so Z64 programs and programs that mix the two domains compile on the GPU too, whole or
 * as a stream's pieces, in both gate-stream forms (the forms concern the GF(2) ops only).  The circuit is again the host compiler's
 * field by field.  Still compiled on the host, with its error codes: a program with a B2A op or with a SizeHint that grows a wire
 * count, RV_COMPILE_KEEP_WIRES, RV_LAZY_K, an op-list error in either domain, more than 2^16 dependency rounds in either domain, and
 * a plain (not RV_COMPILE_WHOLE_PROVER) whole-program compile of a deep, narrow circuit that the host compiler recompiles with lazy
 * sums.  Without this bit every call decides as it did before the bit existed. */
#define RV_COMPILE_DEVICE_Z64 8u /* with RV_COMPILE_DEVICE: the device compiler also takes Z64 ops and SizeHint ops that grow nothing */
/* RV_COMPILE_DEVICE_B2A, only together with RV_COMPILE_DEVICE | RV_COMPILE_DEVICE_Z64 (RV_E_ARG otherwise, with a message that names
 * the missing bit; rv_circuit_compile_device implies RV_COMPILE_DEVICE and still needs RV_COMPILE_DEVICE_Z64): the device compiler
 * also takes B2A ops, the one op kind that joins the two domains, so programs that really use both compile on the GPU -- whole, in
 * both gate-stream forms, or as a stream's pieces (every piece then goes to the device compiler, and a device feed copies none to the
 * host).  A B2A op is expanded where the list is split by domain: its 442 GF(2) steps (64 fresh masks, the 63 Mul and 250 Xor of the
 * ripple-carry adder, 64 recorded reconstructions) join the GF(2) ops in the host compiler's order, and its Gate64 sits one level
 * above its deepest reconstruction.  The circuit is again the host compiler's field by field.  Still compiled on the host, with its
 * error codes: RV_COMPILE_KEEP_WIRES, a SizeHint that grows a wire count, RV_LAZY_K, any op-list error (a B2A whose result wire or
 * whose 64 source wires are out of range included), more than 2^16 dependency rounds in either domain, an expanded GF(2) list of
 * 2^28 entries or more, and a plain (not RV_COMPILE_WHOLE_PROVER) whole-program compile of a deep, narrow circuit -- one adder is
 * about 190 levels deep, so of the B2A programs only wide ones are final in the plain form; the lazy-sum form takes them all.
 * The value is 32, not 16: 16 stays an unknown bit (RV_E_ARG, "unknown flag bits"), as callers and tests written against the
 * previous flag set expect of the first bit above it.  Without this bit every call decides as it did before the bit existed. */
#define RV_COMPILE_DEVICE_B2A 32u /* with RV_COMPILE_DEVICE | RV_COMPILE_DEVICE_Z64: the device compiler also takes B2A ops */
/* RV_COMPILE_DEVICE_KEEP_WIRES, only together with RV_COMPILE_KEEP_WIRES and RV_COMPILE_DEVICE (RV_E_ARG otherwise, with a message
 * that names what is missing; rv_circuit_compile_device implies RV_COMPILE_DEVICE): RV_COMPILE_KEEP_WIRES no longer sends the program
 * to the host compiler.  The device compiler counts one more read of every written wire's final value, so the sum that makes it is
 * not dropped as unread, and builds both wire tables where the circuit lives -- every GF(2) wire's final form (rows numbered as gate
 * operands are; a never-written wire is the zero form) and every Z64 wire's final SSA id -- so rv_evaluate / rv_evaluate_batch of an
 * op list that sits in device memory need no host compile.  It combines freely with RV_COMPILE_WHOLE_PROVER, RV_COMPILE_DEVICE_Z64
 * and RV_COMPILE_DEVICE_B2A, and every other fallback rule of those bits stands.  The circuit is the host compiler's
 * RV_COMPILE_KEEP_WIRES circuit field by field.  For whole programs only: rv_ctx_set_compile_flags, rv_stream_set_compile_flags and
 * rv_eval_stream_set_compile_flags answer "unknown flag bits" for it (a stream's pieces write their wires back instead).  The value
 * is 128: 16 and 64 stay unknown bits.  Without this bit every call decides as it did before the bit existed. */
#define RV_COMPILE_DEVICE_KEEP_WIRES 128u /* with RV_COMPILE_KEEP_WIRES | RV_COMPILE_DEVICE: the device compiler keeps the wires' final values too */
/* The same for an op array already in device memory (n_ops packed 24-byte records on the context's device, e.g. a torch tensor);
 * the caller keeps ownership of d_ops and must have finished writing it.  A program the device path does not take is copied to the
 * host and compiled there. */
int rv_circuit_compile_device(rv_ctx *ctx, const rv_op *d_ops, size_t n_ops, size_t z64_wires, size_t gf2_wires, uint32_t flags,
                              rv_circuit **out);
/* Compile flags of the context's own compiles (rv_prove_ops, rv_verify_ops); 0 (the default), RV_COMPILE_DEVICE,
 * RV_COMPILE_DEVICE | RV_COMPILE_DEVICE_Z64 (the cold compiles of Z64 and mixed programs on the device too) or
 * RV_COMPILE_DEVICE | RV_COMPILE_DEVICE_Z64 | RV_COMPILE_DEVICE_B2A (those of programs with B2A ops too).  Under
 * RV_COMPILE_DEVICE rv_prove_ops compiles the plain form on the device instead of the RV_COMPILE_WHOLE_PROVER one: the same proof
 * bytes, a faster first proof of a wide circuit, 2-4 % slower proofs of it afterwards.  (The device compiler builds the
 * RV_COMPILE_WHOLE_PROVER form too -- rv_circuit_compile_ex with both flags --; rv_prove_ops does not ask it for that form,
 * DESIGN.md 14.)  rv_verify_ops keeps the plain form either way.  RV_E_ARG for any other bit, RV_COMPILE_WHOLE_PROVER included. */
int rv_ctx_set_compile_flags(rv_ctx *ctx, uint32_t flags);
void rv_circuit_destroy(rv_circuit *c);

typedef struct rv_circuit_info {
    uint64_t n_ops;
    uint64_t gf2_inputs, gf2_muls, gf2_asserts, gf2_linear; /* linear = gates with no transcript output */
    uint64_t gf2_masks;                                     /* ShareGen::next() calls per repetition       */
    uint64_t z64_inputs, z64_muls, z64_asserts, z64_linear, z64_masks;
    uint64_t b2a;
    uint64_t levels;         /* dependency levels = kernel launches of the interpreter */
    uint64_t device_bytes;   /* HBM held by the compiled circuit                       */
    uint64_t scratch_bytes;  /* HBM a full 256-repetition prove needs on top           */
    uint64_t compile_us;     /* host time of the gate-stream compiler                  */
    uint64_t upload_us;      /* allocation + host-to-device copy of the compiled gate stream (device_bytes), synchronised */
    /* ABI 4: share rows the GF(2) interpreter reads as gate operands (a Mul's two fresh mask rows not counted) and
     * computed rows it writes (materialised linear gates), per proof -- they depend on how linear gates were compiled */
    uint64_t gf2_operand_rows, gf2_rows_written;
} rv_circuit_info; /* (no size field: this struct does not grow -- later additions get getters of their own, like the one below) */
int rv_circuit_get_info(const rv_circuit *c, rv_circuit_info *info);
/* *on_device = 1 when the device compiler (RV_COMPILE_DEVICE, rv_circuit_compile_device) made this circuit, 0 when the host compiler
 * did -- because the flag was not set, or because the device path handed the program back.  The circuit is the same either way. */
int rv_circuit_compiled_on_device(const rv_circuit *c, int *on_device);
/* ABI 7 (ABI 6 had it as a field of rv_circuit_info): page-locked host memory rv_prove's early-corrections path stages this
 * circuit's corrections vectors in (0: the path does not apply to the circuit), as the RV_EARLY_* environment stands at the call.
 * Allocated once per context, on the first proof that takes the path (its first mapping costs 0.15 - 1.5 s), and kept;
 * RV_EARLY=0 proves without it.  The query builds a plan of its own and leaves the circuit's (made by its first proof) alone. */
int rv_circuit_early_staging_bytes(const rv_circuit *c, uint64_t *bytes);

/* ---- Proof::new -------------------------------------------------------------------
 * wit_gf2: one byte per GF(2) witness element (0/1), consumed by Input gates in order
 *          (the reference takes Vec<bool>);  wit_z64: u64 witness elements.
 * seeds:   256 x 16 bytes, one per repetition (the reference draws them from OsRng,
 *          proof/mod.rs:131-134).  NULL => drawn from the OS (getrandom).
 * *proof:  bincode(Proof), allocated by the library, released with rv_free.  Proofs of a megabyte and more come in
 *          page-locked memory from a small process-wide pool (the device-to-host copy runs at PCIe rate and
 *          rv_free recycles the buffer for the next proof); the pointer is ordinary readable/writable host memory.
 * Memory the call leaves on the context (kept for the next proof, released by rv_ctx_destroy): the device arena's cached blocks
 *          (rv_circuit_info::scratch_bytes), and -- for circuits that take the early-corrections path, pure GF(2) with >= 2^21
 *          Mul gates or pure Z64 with >= 2^17 -- page-locked staging of rv_circuit_early_staging_bytes() (160 MB for the
 *          10^7-gate GF(2) benchmark circuit, 2 GB for the 10^6-MUL Z64 one; its first mapping costs 0.15 - 1.5 s inside the first
 *          such proof) plus as much device memory for GF(2); RV_EARLY=0 in the environment proves without it. */
int rv_prove(rv_ctx *ctx, const rv_circuit *c, const uint8_t *wit_gf2, size_t n_gf2, const uint64_t *wit_z64,
             size_t n_z64, const uint8_t *seeds, uint8_t **proof, size_t *proof_len);

/* ---- Proof::new / Proof::verify on the raw op list (SURVEY 8(b)'s signature) ------------------------------
 * What the reference's own entry points take (proof/mod.rs:119-125,224-232: the op list, the witness, (z64, gf2) wire
 * counts): compile (RV_COMPILE_WHOLE_PROVER for the prover) + prove / verify + release, in one call -- the form a drop-in for
 * a single Proof::new uses.  The compile runs on several host threads (csrc/compile_par.cpp): a circuit the library has not
 * seen costs ~0.1 s per 10^7 gates before its first proof.  The context keeps the circuits these two calls compile and finds them
 * again BY CONTENT: every kept circuit owns a copy of the op array it was compiled from (24 bytes per op of host memory) and a hit is
 * a full comparison of the caller's array against it on host threads (~4 ms per 10^7 ops) -- no hash is trusted, so neither the prover
 * nor the verifier can be handed another statement's gate stream (round 5 keyed the cache by an unkeyed 128-bit hash: constructible
 * collisions made rv_verify_ops accept a proof for a different circuit).  A second Proof::new on the same op list finds its gate stream
 * on the device and costs the comparison plus a proof (rv_prove's early-corrections path included).  At most RV_OPS_CACHE circuits per
 * context (environment, default 2; the least recently used one leaves BEFORE a new one is compiled; 0: nothing is kept), released by
 * rv_ctx_destroy or rv_ctx_ops_cache_clear.  Both calls therefore MUTATE the context (one call at a time per context, like every entry
 * point).  Callers that hold a circuit anyway compile it once (rv_circuit_compile_ex) and call rv_prove: no comparison.
 * flags of rv_verify_ops: as rv_verify_ex. */
int rv_prove_ops(rv_ctx *ctx, const rv_op *ops, size_t n_ops, const uint8_t *wit_gf2, size_t n_gf2, const uint64_t *wit_z64, size_t n_z64,
                 size_t z64_wires, size_t gf2_wires, const uint8_t *seeds, uint8_t **proof, size_t *proof_len);
int rv_verify_ops(rv_ctx *ctx, const rv_op *ops, size_t n_ops, size_t z64_wires, size_t gf2_wires, const uint8_t *proof, size_t proof_len,
                  uint32_t flags, int *ok);
int rv_ctx_ops_cache_clear(rv_ctx *ctx); /* releases the circuits rv_prove_ops / rv_verify_ops keep (ABI 7) */

/* ---- Proof::new with the openings left in device memory ------------------------------------
 * The whole prover (commit, Fiat-Shamir, openings) with ONE host synchronisation, for callers that keep working on
 * the GPU (bench.py's HBM-resident metric): writes [gf2 online | gf2 preprocessing | z64 online | z64 preprocessing]
 * (lens[4]) to dst_device and returns comm and the opening map; rv_assemble_proof frames them as bincode(Proof).
 * Capacity of dst_device: 40 * record sizes (rv_circuit_record_sizes) + 2 * 216 * 48.  seeds must not be NULL. */
int rv_prove_device(rv_ctx *ctx, const rv_circuit *c, const uint8_t *wit_gf2, size_t n_gf2, const uint64_t *wit_z64,
                    size_t n_z64, const uint8_t *seeds, void *dst_device, uint8_t comm[RV_HASH_SIZE],
                    uint8_t omit[RV_TOTAL_REPS], size_t lens[4]);

/* ---- many proofs of one circuit ------------------------------------------------------------
 * `batch` independent Proof::new calls (witness b at wit_gf2 + b*n_gf2 / wit_z64 + b*n_z64, seeds b at
 * seeds + b*256*16, NULL => OS randomness) executed together; the reference reaches the same goal with one rayon
 * task per proof.  Small and medium circuits: every dependency level of the circuit AND every per-proof phase (keys,
 * masks, digests, Fiat-Shamir, openings) is launched once for the whole batch (gridDim.y = proof) -- this is what
 * makes deep, narrow circuits (AES, SHA-256: thousands of levels of a few gates, latency-bound for one proof) use the
 * GPU.  Circuits of 2^20 gates and more fill the GPU on their own: there a few host threads keep several proofs in
 * flight so that one proof's VALU-bound phases, another's memory-bound interpreter and a third one's PCIe copy overlap.
 * proofs[b] / proof_lens[b] as rv_prove (rv_free each, exactly once).  The proofs of a call are slices of one
 * page-locked buffer that goes back to the library's pool when the last of them has been freed (RV_BATCH_COPY_OUT=1:
 * separately malloc'ed buffers, small-circuit path only).  Each proof is byte-identical to what rv_prove returns for
 * the same witness and seeds.  Z64 and mixed circuits below 2^20 gates (GF(2) and Z64 gates counted together) take the
 * one-pass path as well, their Z64 levels through k_interp64_b, in chunks of what fits in device memory; larger Z64 / mixed
 * circuits prove one rv_prove per proof. */
int rv_prove_batch(rv_ctx *ctx, const rv_circuit *c, size_t batch, const uint8_t *wit_gf2, size_t n_gf2,
                   const uint64_t *wit_z64, size_t n_z64, const uint8_t *seeds, uint8_t **proofs, size_t *proof_lens);

/* rv_prove_batch with the proofs left in device memory.  Witnesses and seeds as rv_prove_batch (seeds must not be NULL, as with
 * rv_prove_device).  dst_device + b*stride receives bincode(Proof) for witness b, repetition counts in place: the bytes
 * rv_verify_device and rv_verify_batch_device take, byte-identical to rv_prove_batch's proof b for the same witnesses and seeds.
 * The proof length is the same for every proof of a circuit,
 *     32 + 4*8 + 40 * (gf2 + z64 online record sizes, rv_circuit_record_sizes) + 2 * 216 * 48,
 * and is returned in *proof_len (also when the buffer is refused); bytes between it and `stride` are unspecified.
 * dst_device: memory of the context's device, 256-byte aligned; stride: a multiple of 256, at least the proof length;
 * batch * stride inside the allocation -- RV_E_ARG otherwise, before anything runs.
 * The path is rv_prove_batch's (the one-pass path, Z64 chunks by free memory and RV_BATCH_MAX), and so are the error codes;
 * per pass only the proofs' error words cross to the host, in one copy with one synchronisation.  A batch of one and circuits
 * from RV_BATCH_BIG_GATES on are proved one proof after another on the context's stream, each opened straight into its place:
 * sequential on purpose -- the worker threads of rv_prove_batch's large-circuit path exist to hide a proof's copy over PCIe
 * behind the next proof's kernels, and this call makes no such copy. */
int rv_prove_batch_device(rv_ctx *ctx, const rv_circuit *c, size_t batch, const uint8_t *wit_gf2, size_t n_gf2,
                          const uint64_t *wit_z64, size_t n_z64, const uint8_t *seeds /* batch x 256 x 16, not NULL */,
                          void *dst_device, size_t stride, size_t *proof_len);

/* ---- cleartext evaluation (mcircuit::evaluate_composite_program, re-exported at src/lib.rs:6; the CLI's `oneshot`) ----
 * Evaluates the circuit on the witness in the clear, on the GPU: no shares, no transcripts.  A failing AssertZero is not an error:
 * the call returns RV_OK and the status says which assertions do not hold.  gf2_values / z64_values (NULL: not wanted) receive the
 * first gf2_wires / z64_wires wires' values at the end of the program (the wire counts the circuit was compiled with; one byte 0/1
 * per GF(2) wire), which needs a circuit compiled with RV_COMPILE_KEEP_WIRES (RV_E_ARG otherwise).  Op lists with Random ops have no
 * single cleartext value: RV_E_UNSUPPORTED.  A witness shorter than the Input ops: RV_E_WITNESS_SHORT (as rv_prove).
 * rv_evaluate_batch: `batch` witnesses at once (witness b at wit_gf2 + b*n_gf2 / wit_z64 + b*n_z64, values at gf2_values +
 * b*gf2_wires / z64_values + b*z64_wires, status st[b]); each result equals rv_evaluate's for that witness.  Runs on the context's
 * stream; a batch that does not fit in half of the free device memory is evaluated in parts. */
typedef struct rv_eval_status {
    uint64_t n_failed;        /* AssertZero ops that do not hold */
    uint64_t first_failed_op; /* op-list index of the first failing AssertZero in program order; UINT64_MAX if none */
} rv_eval_status;
int rv_evaluate(rv_ctx *ctx, const rv_circuit *c, const uint8_t *wit_gf2, size_t n_gf2, const uint64_t *wit_z64, size_t n_z64,
                uint8_t *gf2_values, uint64_t *z64_values, rv_eval_status *st);
int rv_evaluate_batch(rv_ctx *ctx, const rv_circuit *c, size_t batch, const uint8_t *wit_gf2, size_t n_gf2, const uint64_t *wit_z64,
                      size_t n_z64, uint8_t *gf2_values, uint64_t *z64_values, rv_eval_status *st);

/* ---- witnesses taken from device memory; evaluation results left there ----------------------
 * For a caller who computes witnesses on the GPU and filters them by evaluation before proving: no witness byte crosses PCIe in
 * either direction.  A descriptor names the witnesses; every pointer in it is memory of the context's device.  Witness b of a batch
 * starts at gf2 + b*stride_gf2 (bytes, one byte per bit) and z64 + b*stride_z64 (words); the calls that take one witness ignore the
 * strides, and so does a batch of one.  The caller has finished writing the witnesses before the call; the library does not write
 * them and no longer reads them when the call returns.
 *
 * Each _wdev prover is its host-witness sibling -- the same paths (one-pass batch, Z64 chunks, worker threads, one by one, early
 * corrections), the same error codes, and proofs byte-identical to the sibling's for the same witness bytes and seeds: only the
 * copy that brings the witness to where the kernels read it starts in device memory.
 *
 * Refused with RV_E_ARG before anything is launched: a NULL descriptor; a pointer that is not memory of the context's device, whose
 * range leaves its allocation (where the runtime can tell) or that is misaligned (gf2: 1, z64: 8, d_z64_values: 8, d_status: 16
 * bytes); a stride smaller than its n when batch > 1; a witness range that overlaps dst_device or an output buffer; NULL seeds on
 * the calls whose siblings refuse them.  RV_E_WITNESS_SHORT as the siblings. */
typedef struct rv_dev_witness {
    const uint8_t *gf2; /* n_gf2 bytes per witness */
    size_t n_gf2;
    size_t stride_gf2;   /* bytes between two witnesses' first bits */
    const uint64_t *z64; /* n_z64 words per witness, 8-byte aligned */
    size_t n_z64;
    size_t stride_z64;   /* words between two witnesses' first words */
} rv_dev_witness;
int rv_prove_wdev(rv_ctx *ctx, const rv_circuit *c, const rv_dev_witness *w, const uint8_t *seeds, uint8_t **proof, size_t *proof_len);
int rv_prove_device_wdev(rv_ctx *ctx, const rv_circuit *c, const rv_dev_witness *w, const uint8_t *seeds, void *dst_device,
                         uint8_t comm[RV_HASH_SIZE], uint8_t omit[RV_TOTAL_REPS], size_t lens[4]);
int rv_prove_batch_wdev(rv_ctx *ctx, const rv_circuit *c, size_t batch, const rv_dev_witness *w, const uint8_t *seeds,
                        uint8_t **proofs, size_t *proof_lens);
int rv_prove_batch_device_wdev(rv_ctx *ctx, const rv_circuit *c, size_t batch, const rv_dev_witness *w, const uint8_t *seeds,
                               void *dst_device, size_t stride, size_t *proof_len);
/* rv_evaluate_batch with the witnesses read in device memory, the statuses written to device memory (d_status[b], the 16-byte
 * rv_eval_status; first_failed_op UINT64_MAX when every assertion holds) and values written for chosen wires only:
 * d_gf2_values[b*n_sel_gf2 + i] = the final bit of wire sel_gf2[i], d_z64_values[b*n_sel_z64 + i] = the word of wire sel_z64[i].
 * sel_gf2 / sel_z64 are host arrays; they may be unsorted and may repeat.  A NULL values pointer: that domain is not wanted.  A values
 * pointer with sel NULL and n_sel 0: every wire, in order (rv_evaluate_batch's meaning).  Values need RV_COMPILE_KEEP_WIRES (RV_E_ARG
 * otherwise); an index at or beyond the circuit's wire count: RV_E_WIRE_OOB, before anything is launched.  Parts as
 * rv_evaluate_batch (half of the free memory, RV_EVAL_PART), each writing its slice of the caller's buffers; no result is copied to
 * the host, and the call waits for the device once, at the end. */
int rv_evaluate_batch_device(rv_ctx *ctx, const rv_circuit *c, size_t batch, const rv_dev_witness *w, const uint32_t *sel_gf2,
                             size_t n_sel_gf2, const uint32_t *sel_z64, size_t n_sel_z64, uint8_t *d_gf2_values, uint64_t *d_z64_values,
                             rv_eval_status *d_status);

/* ---- cleartext evaluation of a gate stream with bounded device memory (the streaming evaluator) ----
 * rv_evaluate_batch over an op list fed in pieces, as the streaming prover takes it: no compiled circuit, no keep-wires flag.
 *     rv_eval_stream_begin(ctx, z64_wires, gf2_wires, batch, max_chunk_ops, &s)
 *     rv_eval_stream_feed(s, ops_0, ...) ... rv_eval_stream_feed(s, ops_k, ...)
 *     rv_eval_stream_finish(s, gf2_values, z64_values, st)
 *     rv_eval_stream_abort(s)             releases the stream (also after a finish or an error)
 * A feed carries, for each witness b of the batch, the witness elements its Input gates consume, in order, at wit_gf2 + b*n_gf2 and
 * wit_z64 + b*n_z64 (more may be passed; RV_E_WITNESS_SHORT if fewer).  A feed longer than max_chunk_ops (0 = 2^18) is cut into
 * device chunks as rv_stream_feed cuts it.  A Random op gives RV_E_UNSUPPORTED (as rv_evaluate), and so does a SizeHint that grows
 * the wire counts given at begin (as rv_stream_feed); compile errors keep their codes (RV_E_WIRE_OOB, RV_E_BAD_OP).  After an error
 * the stream only accepts rv_eval_stream_abort.  A feed returns without waiting for the GPU.
 * finish: st[b] is what rv_evaluate_batch returns for witness b and the concatenated op list -- n_failed counts the failing
 * AssertZero ops of all chunks, first_failed_op is the index in the whole op list of the first one in program order (both domains;
 * a failing assertion is a result, not an error).  gf2_values ([batch][gf2_wires] bytes 0/1) and z64_values ([batch][z64_wires])
 * are nullable and receive every wire's final value; a wire that is never written reads 0.  finish may be called once.
 * Device memory: the wire store -- gf2_wires * ceil(batch/32) * 4 + (1 + z64_wires) * batch * 8 bytes plus 28 status bytes per
 * witness -- and one chunk, independent of the number of ops.  A wire store larger than half of the free device memory gives
 * RV_E_NOMEM at begin, before anything is allocated (the batch is not split: run several streams). */
typedef struct rv_eval_stream rv_eval_stream;
typedef struct rv_eval_stream_info {
    uint64_t n_ops, chunks, levels;
    uint64_t wire_store_bytes;  /* HBM held for the carried wires (and status words) of all witnesses */
    uint64_t peak_chunk_bytes;  /* largest chunk's working set (rows, SSA slots, gate records, witness words) */
} rv_eval_stream_info;
int rv_eval_stream_begin(rv_ctx *ctx, size_t z64_wires, size_t gf2_wires, size_t batch, size_t max_chunk_ops, rv_eval_stream **out);
/* As rv_stream_set_compile_flags (below): 0, RV_COMPILE_DEVICE, RV_COMPILE_DEVICE | RV_COMPILE_DEVICE_Z64 or the latter with
 * RV_COMPILE_DEVICE_B2A, before the first feed; the context's flags are the default. */
int rv_eval_stream_set_compile_flags(rv_eval_stream *s, uint32_t flags);
int rv_eval_stream_feed(rv_eval_stream *s, const rv_op *ops, size_t n_ops, const uint8_t *wit_gf2, size_t n_gf2, const uint64_t *wit_z64,
                        size_t n_z64);
/* rv_eval_stream_feed for an op array in the memory of the stream's device (rv_stream_feed_device's conventions; the witnesses
 * stay in host memory -- rv_eval_stream_feed_wdev, below, reads them in device memory): the same statuses and values. */
int rv_eval_stream_feed_device(rv_eval_stream *s, const rv_op *d_ops, size_t n_ops, const uint8_t *wit_gf2, size_t n_gf2,
                               const uint64_t *wit_z64, size_t n_z64);
int rv_eval_stream_finish(rv_eval_stream *s, uint8_t *gf2_values, uint64_t *z64_values, rv_eval_status *st);
int rv_eval_stream_get_info(const rv_eval_stream *s, rv_eval_stream_info *info);
void rv_eval_stream_abort(rv_eval_stream *s);
/* begin + one feed of an op array that already sits in host memory + finish; info (nullable): the stream's final figures */
int rv_evaluate_streaming(rv_ctx *ctx, const rv_op *ops, size_t n_ops, size_t z64_wires, size_t gf2_wires, size_t batch,
                          const uint8_t *wit_gf2, size_t n_gf2, const uint64_t *wit_z64, size_t n_z64, size_t max_chunk_ops,
                          uint8_t *gf2_values, uint64_t *z64_values, rv_eval_status *st, rv_eval_stream_info *info);

/* ---- Proof::verify ----------------------------------------------------------------
 * Verification is STRICT by default (flags 0, rv_verify): on top of the reference's check (*ok = 0 when a ProofSingle
 * has the wrong number of repetitions or the recomputed commitment differs) it closes the two soundness gaps of the
 * reference verifier:
 *   - every AssertZero of the 40 opened repetitions must reconstruct to zero -- VerifierTranscriptOnline.okay
 *     (src/transcript/verifier/online.rs:21,117,175-177), which the reference computes and never reads, so
 *     its Proof::verify accepts a proof of an unsatisfied circuit;
 *   - every online record's `omit` must equal the player the challenge omits -- the reference only checks which
 *     repetitions are opened (src/proof/mod.rs:292-302: contains_key), never by whom.
 * RV_VERIFY_REFERENCE_COMPAT switches both extra checks off: *ok is then exactly what the reference's Proof::verify
 * returns (byte-compatibility tests; never for untrusted proofs).  RV_VERIFY_STRICT is accepted and means flags 0;
 * both bits together are RV_E_ARG.
 * Bytes that cannot be parsed as a Proof, unequal GF(2) opening lengths inside a verifier group, or an
 * `omit` value >= 8 return RV_E_PROOF_MALFORMED (the reference panics / is UB). */
#define RV_VERIFY_STRICT 1u
#define RV_VERIFY_REFERENCE_COMPAT 2u
int rv_verify(rv_ctx *ctx, const rv_circuit *c, const uint8_t *proof, size_t proof_len, int *ok);
int rv_verify_ex(rv_ctx *ctx, const rv_circuit *c, const uint8_t *proof, size_t proof_len, uint32_t flags, int *ok);

/* ---- Proof::verify on proof bytes in device memory ------------------------------------------
 * rv_verify_device: d_proof is proof_len bytes of bincode(Proof) in the memory of the context's device (e.g. a torch tensor); the
 * caller keeps ownership and must have finished writing it (rv_circuit_compile_device's conventions).  flags: as rv_verify_ex.
 * DEFINITION: the return code and *ok are exactly those of rv_verify_ex(ctx, c, a host copy of the same bytes, proof_len, flags, ok),
 * for every byte string -- truncated, wrong repetition counts, altered vector lengths, trailing bytes.
 * rv_verify_sections_device: d_sections is what rv_prove_device, rv_shard_open_self or rv_shard_open_into wrote for a shard of all
 * 256 repetitions -- [gf2 online | gf2 preprocessing | z64 online | z64 preprocessing], contiguous, lens[4] -- and comm (host
 * memory) the proof's commitment.  DEFINITION: the return code and *ok are those of rv_verify_ex on the byte string
 *     comm | LE64(40) | section 0 | LE64(216) | section 1 | LE64(40) | section 2 | LE64(216) | section 3
 * (what rv_assemble_proof frames from the same sections).
 * Both: RV_E_ARG for a pointer that is not 16-byte aligned, that is host memory, or memory of another device.  NO PADDING is asked
 * of the caller: a well-framed proof is read inside [d_proof, d_proof + proof_len) only.  (The GF(2) unpack kernel's aligned
 * 32-bit loads reach up to 3 bytes in front of a vector and 3 behind it; at least 137 bytes of the record lie in front of every
 * vector, and 8 or more bytes of the proof behind it -- the next length field, or the count and the preprocessing records that
 * follow every online section.  The Z64 unpack kernel loads bytes of the vector only.)
 * How: one small kernel walks the framing (at most 80 records; a repetition count other than 40 / 216 stops it at once), the host
 * reads back its status with comm and the 80 omit bytes, a second kernel builds the verifier's slot arrays in device memory and the
 * verifier runs on them with the vectors read in place: no proof byte crosses to the host and rv_hook_verify_proof_bytes does not
 * move.  Bytes the walk refuses (they run out; a count is not 40 / 216; a section does not end where its records do; a group's
 * records break the rules rv_verify_ex answers RV_E_PROOF_MALFORMED for) are copied to the host and handed to rv_verify_ex -- and
 * only those: a well-framed proof whose records pass those rules takes the device path whatever its vector lengths. */
int rv_verify_device(rv_ctx *ctx, const rv_circuit *c, const uint8_t *d_proof, size_t proof_len, uint32_t flags, int *ok);
int rv_verify_sections_device(rv_ctx *ctx, const rv_circuit *c, const uint8_t comm[RV_HASH_SIZE], const uint8_t *d_sections,
                              const size_t lens[4], uint32_t flags, int *ok);

void rv_free(void *p);

/* ---- streaming prover --------------------------------------------------------
 * The reference's README promises "a streaming interface" over its single-pass just-in-time preprocessing
 * (/root/reference/README.md:14,38; src/generator/share.rs:54-65), while the surveyed source keeps every
 * reconstruction and correction of all repetitions until the challenge (src/transcript/prover.rs:29-31,211,217).
 * Here the gate stream is fed in pieces and device memory is bounded by
 *     the wire store (one share row per GF(2) wire INDEX, one slot per Z64 wire index -- the reference's own
 *     `wires` vectors, sized by wire_counts) + one chunk's working set + the proof itself,
 * independent of the number of gates: transcripts are hashed chunk by chunk into incremental BLAKE3 trees and
 * dropped.  Because the omitted players are only known after the commitment, the SAME ops are fed twice:
 *
 *     rv_stream_begin(ctx, z64_wires, gf2_wires, seeds, max_chunk_ops, &s)
 *     rv_stream_feed(s, ops_0, ...) ... rv_stream_feed(s, ops_k, ...)      pass 1: commitments
 *     rv_stream_commit(s, comm)                                            Fiat-Shamir challenge
 *     rv_stream_feed(s, ops_0, ...) ... rv_stream_feed(s, ops_k, ...)      pass 2: openings of the 40 challenged reps
 *     rv_stream_finish(s, &proof, &len)        bincode(Proof), byte-identical to rv_prove's for the same seeds
 *     rv_stream_abort(s)                       releases the stream (also after a finish or an error)
 *
 * The pieces of pass 2 need not be cut where those of pass 1 were, but their concatenation must be the same op
 * list and the same witness (both digested as they are fed, also when pass 1's compiled chunk is reused; checked at
 * finish: RV_E_ARG).  wit_gf2 / wit_z64 of a feed are the witness elements its Input gates
 * consume, in order (more may be passed; RV_E_WITNESS_SHORT if fewer).  A feed longer than max_chunk_ops
 * (0 = 2^18) is cut into device chunks of that size (a long feed of chunks >= 2^16 ops starts with pieces of 1/8, 1/4, 1/2).  SizeHint ops may not grow the wire counts given at begin
 * (RV_E_UNSUPPORTED).  After an error the stream only accepts rv_stream_abort. */
int rv_stream_begin(rv_ctx *ctx, size_t z64_wires, size_t gf2_wires, const uint8_t *seeds /* 256 x 16 or NULL */,
                    size_t max_chunk_ops, rv_stream **out);
/* Where the stream's pieces are compiled.  A stream takes the context's flags (rv_ctx_set_compile_flags) when it begins; this call
 * overrides them before the first feed: 0 = on host worker threads (the default), RV_COMPILE_DEVICE = every all-GF(2) piece is
 * uploaded and compiled on the GPU (the chunk mode of the device compiler: the same chunk, field by field), its gate records and
 * ordinal tables staying in device memory; a piece the device path hands back (Z64 / B2A / SizeHint ops, an op-list error) is compiled
 * on the host, with the host compiler's result or error code.  RV_COMPILE_DEVICE | RV_COMPILE_DEVICE_Z64 = the same for every piece
 * without a B2A op: Z64 and mixed pieces are compiled on the GPU too and their Z64 records stay in device memory like the GF(2) ones;
 * handed back are B2A pieces, op-list errors (a SizeHint that grows a wire count is one in a stream) and chains deeper than 2^16
 * rounds.  RV_COMPILE_DEVICE | RV_COMPILE_DEVICE_Z64 | RV_COMPILE_DEVICE_B2A = every piece goes to the device compiler, B2A
 * pieces too; handed back are op-list errors and chains deeper than 2^16 rounds.  The proofs, answers and values are the same bytes
 * either way.  On a
 * batch handle (rv_stream_begin_batch, rv_stream_verify_begin_batch) it holds for the whole batch.  RV_E_ARG: NULL handle, any other
 * bit, or a call after the first feed. */
int rv_stream_set_compile_flags(rv_stream *s, uint32_t flags);
int rv_stream_feed(rv_stream *s, const rv_op *ops, size_t n_ops, const uint8_t *wit_gf2, size_t n_gf2, const uint64_t *wit_z64,
                   size_t n_z64);
/* rv_stream_feed for an op array that already sits in device memory: d_ops is n_ops packed 24-byte records in the memory of the
 * stream's device (rv_circuit_compile_device's convention: the caller keeps ownership and must have finished writing it; 8-byte
 * aligned, RV_E_ARG otherwise).  Through this call and rv_stream_feed the streams still take their witnesses from host memory, in
 * rv_stream_feed's layouts; rv_stream_feed_wdev (below: "streams in device memory") reads them in device memory, with ops from either
 * side.  Serves every stream rv_stream_feed
 * serves -- single and batch provers in both passes, the streaming verifiers -- and may be mixed freely with it inside one stream
 * and between its passes: the pieces are cut by the same rule, the digests and counters are the same numbers, and every proof,
 * answer, error code and rv_stream_info figure is what rv_stream_feed gives for the same ops.  The op list is not copied to the
 * host: one kernel makes each piece's digest and mask / event counts where the ops are; under RV_COMPILE_DEVICE an all-GF(2) piece
 * is compiled from d_ops in place, and only a piece the host compiler has to read (no RV_COMPILE_DEVICE, Z64 / B2A / SizeHint ops,
 * an op-list error, more than 2^16 rounds; with RV_COMPILE_DEVICE_Z64 a Z64 or mixed piece is compiled in place too, and of these
 * only B2A pieces, errors and over-deep chains remain; with RV_COMPILE_DEVICE_B2A on top only errors and over-deep chains) is copied down, into one of a fixed number of page-locked slots: one per compiling
 * thread plus one, each as long as the feed's longest piece, at most 32 and within 512 MiB (two at least).  The slots belong to the
 * context and stay allocated for its next device feed until rv_ctx_destroy.  Returns when the library no longer reads d_ops. */
int rv_stream_feed_device(rv_stream *s, const rv_op *d_ops, size_t n_ops, const uint8_t *wit_gf2, size_t n_gf2, const uint64_t *wit_z64,
                          size_t n_z64);
int rv_stream_commit(rv_stream *s, uint8_t comm[RV_HASH_SIZE] /* nullable */);
int rv_stream_finish(rv_stream *s, uint8_t **proof, size_t *proof_len);
void rv_stream_abort(rv_stream *s);
/* A promise, made during pass 1: pass 2 will be fed in exactly pass 1's pieces (the same rv_stream_feed calls).  Pass 1 then keeps
 * the transcripts of the stream's LAST chunks on the device, as many as fit a budget (RV_STREAM_KEEP_MB; default an eighth of the
 * device's memory, at most 32 GiB; 0 = none; rv_stream_info.kept_mib), and pass 2 takes the openings of those chunks from them
 * instead of running them a second time: the earlier chunks run twice, as every chunk does without the promise.  Device memory
 * stays bounded by wire store + one chunk + the proof + that budget.  A pass 2 that breaks the promise gets RV_E_ARG from the feed
 * that would have to run a chunk after one that did not.  rv_prove_streaming makes the promise itself. */
int rv_stream_same_cuts(rv_stream *s);
typedef struct rv_stream_info {
    uint64_t n_ops, chunks, levels; /* of pass 1 (running totals while it is in progress) */
    uint64_t gf2_masks, z64_masks, gf2_muls, z64_muls;
    uint64_t wire_store_bytes;  /* HBM held by the carried wires + the largest chunk's rows */
    uint64_t peak_chunk_bytes;  /* largest single chunk's working set (rows, transcripts, gate records) */
    uint64_t hash_state_bytes;  /* incremental BLAKE3 trees + unhashed stream tails */
    uint64_t proof_bytes;       /* 0 before rv_stream_commit */
    uint32_t pass;
    uint32_t kept_mib;          /* most MiB of pass-1 transcripts held for pass 2 (RV_STREAM_KEEP_MB; the field was `reserved`, always 0) */
} rv_stream_info;
int rv_stream_get_info(const rv_stream *s, rv_stream_info *info);
/* Both passes over an op array that already sits in host memory: Proof::new with bounded DEVICE memory.
 * info (nullable) receives the stream's final figures. */
int rv_prove_streaming(rv_ctx *ctx, const rv_op *ops, size_t n_ops, size_t z64_wires, size_t gf2_wires, const uint8_t *wit_gf2,
                       size_t n_gf2, const uint64_t *wit_z64, size_t n_z64, const uint8_t *seeds, size_t max_chunk_ops,
                       uint8_t **proof, size_t *proof_len, rv_stream_info *info);

/* ---- Proof::verify with bounded device memory (the streaming verifier) -----------------------------------------------
 * The reference's verify walks the op list like its prover (proof/mod.rs:259-261,276-278); rv_verify keeps the whole compiled
 * circuit and its rows resident (~6 GB for 10^7 GF(2) gates, ~90 GB for 10^6 Z64 multiplications).  Here the ops are fed in
 * pieces, ONCE (the omitted players are in the proof), and device memory is the streaming prover's: wire store + one chunk +
 * the proof.
 *     rv_stream_verify_begin(ctx, z64_wires, gf2_wires, proof, proof_len, max_chunk_ops, &s)   (proof must outlive the stream)
 *     rv_stream_feed(s, ops_0, n, NULL, 0, NULL, 0) ... rv_stream_feed(s, ops_k, ...)           (no witness)
 *     rv_stream_verify_finish(s, flags, &ok)      flags as rv_verify_ex; ok = what rv_verify_ex answers for the same ops
 *     rv_stream_abort(s)
 * A proof with the wrong repetition counts gives ok = 0 (as rv_verify); a malformed one RV_E_PROOF_MALFORMED at begin. */
int rv_stream_verify_begin(rv_ctx *ctx, size_t z64_wires, size_t gf2_wires, const uint8_t *proof, size_t proof_len, size_t max_chunk_ops,
                           rv_stream **out);
int rv_stream_verify_finish(rv_stream *s, uint32_t flags, int *ok);
/* begin + one feed of an op array that already sits in host memory + finish; info (nullable): the stream's final figures */
int rv_verify_streaming(rv_ctx *ctx, const rv_op *ops, size_t n_ops, size_t z64_wires, size_t gf2_wires, const uint8_t *proof, size_t proof_len,
                        uint32_t flags, size_t max_chunk_ops, int *ok, rv_stream_info *info);

/* ---- batches over one stream: B witnesses (or B proofs) of ONE statement, the op list fed once per pass ------------------------
 * The host work of a chunk (compile, relocation, gate upload) -- what paces a streamed proof -- is done once for the batch; the
 * device work of the chunk is issued for every proof of the batch.
 *     rv_stream_begin_batch(ctx, z64_wires, gf2_wires, B, seeds, max_chunk_ops, &s)   seeds: B x 256 x 16 (rv_prove_batch's layout)
 *                                                                                     or NULL (fresh seeds for every proof)
 *     rv_stream_feed(s, ops, n, wit_gf2, n_gf2, wit_z64, n_z64)   ...   pass 1; witness b at wit_gf2 + b*n_gf2, wit_z64 + b*n_z64
 *                                                                       (n_gf2 / n_z64 per witness: rv_eval_stream_feed's layout)
 *     rv_stream_commit_batch(s, comms)          comms: B x 32 (nullable)
 *     rv_stream_feed(s, ...)                    ...   pass 2: pass 1's op list and every witness again
 *     rv_stream_finish_batch(s, proofs, lens)   proofs[b] (rv_free each) is byte-identical to rv_prove's for witness b and
 *                                               seeds + b*4096, and to rv_stream_* / rv_prove_streaming's
 * rv_stream_feed, rv_stream_same_cuts, rv_stream_get_info and rv_stream_abort take batch streams unchanged.  A batch of 1 is a
 * single stream in every output (the _batch forms also take a stream of rv_stream_begin).  rv_stream_commit, rv_stream_finish and
 * rv_stream_verify_finish on a stream of batch > 1, batch == 0, a null handle or array, and a _batch form on the other kind of
 * stream (prover / verifier) give RV_E_ARG.
 * A failing AssertZero of any witness gives RV_E_WITNESS_INVALID from the feed that holds it (rv_last_error names the first such
 * witness); the stream then only accepts rv_stream_abort.  The witness digests are kept per proof: pass 2 with any witness changed
 * gives RV_E_ARG at finish.  rv_stream_same_cuts keeps a chunk's transcripts for all B proofs or for none, and RV_STREAM_KEEP_MB is
 * the budget of the whole batch.
 * Device memory: B wire stores + one chunk's working set per proof + B proofs (+ the kept budget).  If B > 1 wire stores exceed half
 * of the free device memory, begin gives RV_E_NOMEM before anything is allocated (the batch is not split; a batch of 1 is begun as
 * rv_stream_begin begins a stream).  rv_stream_get_info on a
 * batch: n_ops .. z64_muls are the stream's (every proof's are the same); wire_store_bytes, peak_chunk_bytes, hash_state_bytes,
 * proof_bytes and kept_mib are totals over the batch. */
int rv_stream_begin_batch(rv_ctx *ctx, size_t z64_wires, size_t gf2_wires, size_t batch, const uint8_t *seeds /* batch x 256 x 16, or NULL */,
                          size_t max_chunk_ops, rv_stream **out);
int rv_stream_commit_batch(rv_stream *s, uint8_t *comms /* batch x 32, nullable */);
int rv_stream_finish_batch(rv_stream *s, uint8_t **proofs /* [batch] */, size_t *proof_lens /* [batch] */);
/* both passes over an op array in host memory; wit_gf2 / wit_z64: [batch][n_gf2] / [batch][n_z64]; info (nullable) as above */
int rv_prove_streaming_batch(rv_ctx *ctx, const rv_op *ops, size_t n_ops, size_t z64_wires, size_t gf2_wires, size_t batch,
                             const uint8_t *wit_gf2, size_t n_gf2, const uint64_t *wit_z64, size_t n_z64, const uint8_t *seeds,
                             size_t max_chunk_ops, uint8_t **proofs, size_t *proof_lens, rv_stream_info *info);
/* The batched streaming verifier: ok[b] is what rv_verify_streaming / rv_verify_ex answers for proof b with the same flags.  A proof
 * that cannot be parsed or has the wrong repetition counts gets ok[b] = 0 and the others are verified all the same (rv_verify_batch's
 * rule); a non-zero return is an argument or device error.  The proofs must outlive the stream. */
int rv_stream_verify_begin_batch(rv_ctx *ctx, size_t z64_wires, size_t gf2_wires, size_t batch, const uint8_t *const *proofs,
                                 const size_t *proof_lens, size_t max_chunk_ops, rv_stream **out);
int rv_stream_verify_finish_batch(rv_stream *s, uint32_t flags, int *ok /* [batch] */);
int rv_verify_streaming_batch(rv_ctx *ctx, const rv_op *ops, size_t n_ops, size_t z64_wires, size_t gf2_wires, size_t batch,
                              const uint8_t *const *proofs, const size_t *proof_lens, uint32_t flags, size_t max_chunk_ops,
                              int *ok, rv_stream_info *info);

/* ---- streams in device memory: witnesses in, proofs out, verification in place --------------------------------------------------
 * For a caller whose circuit, witness and proof live on the GPU: with rv_stream_feed_device's ops these calls keep the witness, the
 * proof and the verifier's input off PCIe.  They are pure additions: every other entry point, proof byte and error code is unchanged.
 *
 * rv_stream_feed_wdev / rv_eval_stream_feed_wdev: a feed whose witnesses are read in the memory of the stream's device.  `ops` is a
 * host array (ops_on_device == 0, rv_stream_feed's rules) or device memory (!= 0, rv_stream_feed_device's rules).  `w`: n_gf2 / n_z64
 * are the elements still available to this feed, per witness (more may be passed; fewer: RV_E_WITNESS_SHORT, as the siblings); witness
 * b of a batch stream starts at gf2 + b*stride_gf2 and z64 + b*stride_z64, a single stream and a batch of one ignore the strides.  A
 * verifier stream takes w == NULL or a descriptor with both counts 0; a prover or evaluator stream needs a descriptor.  Checked before
 * anything is launched (RV_E_ARG): the pointers are memory of the stream's device, the ranges lie inside their allocations (where the
 * runtime can tell), alignment 1 (gf2) / 8 (z64), stride >= n when batch > 1.  Every error, these included, is sticky: the stream
 * then only accepts its abort.  Host and device witness feeds may be mixed inside a stream and between its passes, like host and
 * device op feeds: the proof, comm, every rv_stream_info figure and every error code are rv_stream_feed's for the same witness bytes
 * (the position-keyed witness digest that lets finish refuse a pass 2 fed another witness is summed by a kernel for these feeds, and
 * read at commit and at finish).  When the call returns the library no longer reads the witness (rv_eval_stream_feed_wdev therefore
 * waits for the device once, which rv_eval_stream_feed does not). */
int rv_stream_feed_wdev(rv_stream *s, const rv_op *ops, size_t n_ops, int ops_on_device, const rv_dev_witness *w);
int rv_eval_stream_feed_wdev(rv_eval_stream *s, const rv_op *ops, size_t n_ops, int ops_on_device, const rv_dev_witness *w);
/* rv_stream_finish / rv_stream_finish_batch with the proof left in device memory: the same bytes (comm, the four counts, the four
 * sections -- rv_prove's for the same seeds) at dst_device, for a batch at dst_device + b*stride; no proof byte is copied to the host.
 * The single form needs a 16-byte aligned destination (what rv_verify_device accepts) and cap >= rv_stream_info.proof_bytes; the
 * batch form follows rv_prove_batch_device: 256-byte alignment, stride a multiple of 256 and >= the proof length.  A destination
 * that is too small, misaligned, not memory of the stream's device or outside its allocation gives RV_E_ARG with *proof_len = the
 * required length, and the stream is not finished: the caller may call again.  rv_stream_finish_batch_device on a single stream is
 * rv_stream_finish_device with cap = stride; the single form on a batch > 1 gives RV_E_ARG. */
int rv_stream_finish_device(rv_stream *s, void *dst_device, size_t cap, size_t *proof_len);
int rv_stream_finish_batch_device(rv_stream *s, void *dst_device, size_t stride, size_t *proof_len);
/* rv_stream_verify_begin / _begin_batch for proof bytes in the memory of the context's device (16-byte aligned; RV_E_ARG otherwise):
 * the framing is walked where the bytes lie, the verifier's slot arrays are made on the device and the chunks read the vectors from
 * the caller's buffer, which must outlive the stream and must not be written meanwhile.  Only the walk's table crosses to the host
 * (offsets, lengths, the 80 omit bytes, comm).  Feeds, rv_stream_verify_finish(_batch), info and abort are unchanged, and the answer
 * and return code are rv_verify_streaming's on a host copy of the same bytes, for every byte string: bytes that are not a well-framed
 * proof of acceptable records are copied to a host buffer the stream owns and begin as the host form does (RV_E_PROOF_MALFORMED, or
 * ok = 0 for wrong counts; in a batch such a member answers 0 alone).  d_proofs is a host array of device pointers. */
int rv_stream_verify_begin_device(rv_ctx *ctx, size_t z64_wires, size_t gf2_wires, const uint8_t *d_proof, size_t proof_len,
                                  size_t max_chunk_ops, rv_stream **out);
int rv_stream_verify_begin_batch_device(rv_ctx *ctx, size_t z64_wires, size_t gf2_wires, size_t batch,
                                        const uint8_t *const *d_proofs /* host array of device pointers */,
                                        const size_t *proof_lens, size_t max_chunk_ops, rv_stream **out);

/* ---- sharded form (one process per GPU; repetitions [rep_begin, rep_begin+rep_count),
 * both multiples of 8).  rv_prove == commit(0,256) -> combine -> challenge -> open ->
 * assemble.  Between commit and open the caller exchanges the 32-byte per-repetition
 * digests (one all-gather; proof/mod.rs:160-172 is the reference's gather point). */
int rv_shard_commit(rv_ctx *ctx, const rv_circuit *c, const uint8_t *wit_gf2, size_t n_gf2, const uint64_t *wit_z64,
                    size_t n_z64, const uint8_t *seeds /* rep_count x 16 */, uint32_t rep_begin, uint32_t rep_count,
                    rv_shard **out);
/* device pointer to rep_count x 32 digest bytes (valid until rv_shard_destroy), for RCCL */
int rv_shard_digests_device(rv_shard *s, void **dptr);
/* host copy of the same bytes */
int rv_shard_digests(rv_shard *s, uint8_t *out /* rep_count x 32 */);
/* device-to-device copy of the same bytes into caller-owned HBM (e.g. a torch tensor that
 * RCCL will all-gather); complete when the call returns */
int rv_shard_digests_to_device(rv_shard *s, void *dst_device);
/* Opens the shard's repetitions for the full challenge (omit[256], 8 = preprocessing).
 * Returns four blobs: the shard's OpenOnline / OpenPreprocessing records, in ascending
 * repetition order, already in bincode form, for the gf2 and z64 ProofSingle.
 * Each blob is library-allocated (rv_free). */
typedef struct rv_shard_parts {
    uint8_t *gf2_online, *gf2_pre, *z64_online, *z64_pre;
    size_t gf2_online_len, gf2_pre_len, z64_online_len, z64_pre_len;
    uint32_t n_online, n_pre;
} rv_shard_parts;
int rv_shard_open(rv_shard *s, const uint8_t omit[RV_TOTAL_REPS], rv_shard_parts *parts);
void rv_shard_destroy(rv_shard *s);

/* Device-resident variant used by bench.py: leaves the shard's four blobs concatenated
 * in HBM (gf2_online | gf2_pre | z64_online | z64_pre) and returns the device pointer,
 * valid until the shard is destroyed. */
int rv_shard_open_device(rv_shard *s, const uint8_t omit[RV_TOTAL_REPS], void **dptr, size_t lens[4]);
/* Bytes of one OpenOnline record of the gf2 / z64 ProofSingle for this circuit (every record of a
 * section has the same size; an OpenPreprocessing record is always 48 bytes).  Lets every rank
 * compute every other rank's blob sizes from the challenge alone. */
int rv_circuit_record_sizes(const rv_circuit *c, size_t *gf2_online_record, size_t *z64_online_record);
/* Sizes rv_shard_open* will produce for this challenge, without opening */
int rv_shard_open_size(const rv_shard *s, const uint8_t omit[RV_TOTAL_REPS], size_t lens[4]);
/* As rv_shard_open_device, but writes the concatenated blobs into caller-owned HBM
 * (sum of rv_shard_open_size bytes), e.g. a torch tensor handed to RCCL afterwards */
int rv_shard_open_into(rv_shard *s, const uint8_t omit[RV_TOTAL_REPS], void *dst_device, size_t lens[4]);
/* Fiat-Shamir without leaving the device, for a shard that holds ALL 256 repetitions (rep_begin 0, rep_count 256):
 * comm = BLAKE3(digests) (combine_hashes, proof/mod.rs:102-108), the challenge (RandomOracle + challenge_to_opening,
 * crypto/ro.rs:8-20, proof/mod.rs:68-83) and the openings, with no host round trip in between.  Equivalent to
 * rv_shard_digests -> rv_combine_digests -> rv_challenge -> rv_shard_open_into; returns comm and the opening map.
 * dst_device capacity: the sum rv_shard_open_size reports for ANY 40/216 map (sizes do not depend on which
 * repetitions open).  RV_E_ARG for a partial shard. */
int rv_shard_open_self(rv_shard *s, void *dst_device, uint8_t comm[RV_HASH_SIZE], uint8_t omit[RV_TOTAL_REPS], size_t lens[4]);
/* The sharded counterpart: all_digests_device = the 256 x 32 bytes every rank holds on its GPU after the all-gather.
 * Commitment, challenge and this shard's openings without a host round trip; comm / omit as above.  How many of the
 * shard's repetitions open depends on the challenge, so dst_device must hold the worst case:
 *   min(40, rep_count) * (gf2 record + z64 record) + 2 * rep_count * 48 bytes (rv_circuit_record_sizes);
 * lens[4] reports what was written: [gf2 online | gf2 preprocessing | z64 online | z64 preprocessing], contiguous. */
int rv_shard_open_gathered(rv_shard *s, const void *all_digests_device, void *dst_device, uint8_t comm[RV_HASH_SIZE],
                           uint8_t omit[RV_TOTAL_REPS], size_t lens[4]);

/* ---- multi-GPU inside the library ---------------------------------------------------------------
 * The reference fans its 32 packed groups out over a rayon pool INSIDE Proof::new (proof/mod.rs:127-157) and meets
 * again at one point, combine_hashes over the 256 digests (:160-172).  A communicator does the same over GPUs: rank r
 * of `world` (1, 2, 4, 8, 16 or 32) proves repetitions [r*256/world, (r+1)*256/world); the one data-path collective
 * is an ncclAllGather of the 32-byte digests over RCCL/xGMI on the library's own stream; every rank derives the
 * challenge on its GPU and opens its own repetitions; the openings go to rank 0 with ncclSend/ncclRecv straight into
 * their place in the proof.  RCCL is bound at run time (dlopen; RV_RCCL_PATH overrides the search): the library
 * loads without it and reuses a copy the process already has (PyTorch's).
 *   one process per GPU : rank 0 calls rv_comm_unique_id and hands the 128 bytes to the others out of band (MPI,
 *                         torch.distributed, a file); every rank calls rv_comm_create with its own context
 *   one process, n GPUs : rv_comm_create_all(ctxs, n, comms), then rv_prove_multi (a host thread per GPU; its ranks send nothing to
 *                         rank 0: every rank copies its own sections straight into ONE page-locked proof buffer over its own PCIe
 *                         link -- the all-gather of digests stays the only collective)
 * rv_prove_sharded is a COLLECTIVE call: every rank calls it with the same statement and the same 256 seeds (all of
 * them, not only its share; NULL is not allowed -- the ranks could not agree on OS randomness); *proof is set on rank
 * 0 only (NULL / 0 elsewhere) and is byte-identical to rv_prove's.  If one rank fails before the collective the
 * others wait for it: destroy the communicator.  circuits[i] / c must have been compiled on the rank's own context. */
#define RV_COMM_ID_BYTES 128
int rv_comm_unique_id(uint8_t id[RV_COMM_ID_BYTES]);
int rv_comm_create(rv_ctx *ctx, int world, int rank, const uint8_t id[RV_COMM_ID_BYTES], rv_comm **out);
int rv_comm_create_all(rv_ctx *const *ctxs, int n, rv_comm **comms /* [n] */);
void rv_comm_destroy(rv_comm *comm);
int rv_prove_sharded(rv_comm *comm, const rv_circuit *c, const uint8_t *wit_gf2, size_t n_gf2, const uint64_t *wit_z64, size_t n_z64,
                     const uint8_t *seeds /* 256 x 16 */, uint8_t **proof, size_t *proof_len);
/* seeds NULL => drawn once from the OS and shared by the ranks */
int rv_prove_multi(rv_comm *const *comms, const rv_circuit *const *circuits, int n, const uint8_t *wit_gf2, size_t n_gf2,
                   const uint64_t *wit_z64, size_t n_z64, const uint8_t *seeds, uint8_t **proof, size_t *proof_len);

/* combine_hashes (proof/mod.rs:102-108): comm = BLAKE3(h[0] || ... || h[255]) */
int rv_combine_digests(const uint8_t *h /* 256 x 32 */, uint8_t comm[RV_HASH_SIZE]);
/* challenge_to_opening (proof/mod.rs:74-83): omit[r] in 0..7 for the 40 online reps, else 8 */
int rv_challenge(const uint8_t comm[RV_HASH_SIZE], uint8_t omit[RV_TOTAL_REPS]);
/* Concatenates shard parts (ordered by rep_begin) into bincode(Proof) */
int rv_assemble_proof(const uint8_t comm[RV_HASH_SIZE], const rv_shard_parts *parts, size_t n_parts, uint8_t **proof,
                      size_t *proof_len);
/* Verifier side of the sharded form: recomputes the digests of the verifier's
 * repetition slots [slot_begin, slot_begin+slot_count) (slots 0..39 = online openings in
 * proof order, 40..255 = preprocessing openings; proof/mod.rs:234-281), multiples of 8. */
int rv_verify_shard(rv_ctx *ctx, const rv_circuit *c, const uint8_t *proof, size_t proof_len, uint32_t slot_begin,
                    uint32_t slot_count, uint8_t *digests /* slot_count x 32 */);
/* Final check of Proof::verify (proof/mod.rs:283-306) from all 256 slot digests: the reference's check and nothing
 * else (this form has no zero-check input, so it cannot be strict; use the _ex pair below for untrusted proofs). */
int rv_verify_finish(const uint8_t *proof, size_t proof_len, const uint8_t *slot_digests /* 256 x 32 */, int *ok);
/* The sharded form of rv_verify_ex: *zero_checks_ok (nullable) = 0 when an AssertZero of one of this shard's opened
 * repetitions did not reconstruct to zero; AND the shards' values together and hand the result to
 * rv_verify_finish_ex, which (unless RV_VERIFY_REFERENCE_COMPAT) requires it and also compares the records' `omit`
 * with the challenge. */
int rv_verify_shard_ex(rv_ctx *ctx, const rv_circuit *c, const uint8_t *proof, size_t proof_len, uint32_t slot_begin,
                       uint32_t slot_count, uint8_t *digests /* slot_count x 32 */, int *zero_checks_ok);
int rv_verify_finish_ex(const uint8_t *proof, size_t proof_len, const uint8_t *slot_digests /* 256 x 32 */, uint32_t flags,
                        int zero_checks_ok, int *ok);

/* ---- multi-GPU verification inside the library -------------------------------------------
 * The verifier's 256 slots fall into 32 GROUPS of eight (group g = slots 8g .. 8g+7): groups 0..4 are the 40 online records
 * in proof order, groups 5..31 the preprocessing records.  A rank verifies a set of groups; the ranks meet once, in ONE
 * ncclAllGather of their groups' 32-byte slot digests (plus a small trailer with the zero-check flag) on the library's own
 * stream, and every rank then decides on the host (rv_verify_finish_ex over the 256 digests: one BLAKE3 over 8 KiB).
 * Only the proof bytes a rank reads cross PCIe: the records of its online groups (a preprocessing slot needs its seed and
 * online commitment, 48 bytes that travel in the host-side slot arrays).  Nearly all of a proof's bytes are the 40 online
 * records, so the partition deals the 5 online groups round-robin instead of handing them all to rank 0.
 *
 * rv_verify_shard_groups: the digests of groups[0 .. n_groups) (distinct values in 0..31), n_groups * 8 * 32 bytes in the
 * order the groups are given (group g, slot i -> slot 8g+i); zero_checks_ok as rv_verify_shard_ex (which is this call on the
 * groups of its range).  Only the byte ranges of the given online groups' records are copied to the device.  RV_E_ARG for
 * n_groups == 0, a group >= 32, a group given twice or a NULL pointer.  Online groups listed first keep the supplied-value rows
 * narrow (the slot order rv_verify uses). */
int rv_verify_shard_groups(rv_ctx *ctx, const rv_circuit *c, const uint8_t *proof, size_t proof_len, const uint8_t *groups,
                           uint32_t n_groups, uint8_t *digests /* n_groups x 8 x 32 */, int *zero_checks_ok);
/* The groups rank `rank` of `world` verifies (host only, no GPU).  world in {1, 2, 4, 8, 16, 32}: 32/world groups per rank,
 * every group exactly once; the online groups are dealt round-robin (rank r gets online groups r, r+world, ...) and listed
 * first, then the preprocessing groups in ascending order fill every rank, rank after rank, to 32/world.  RV_E_ARG otherwise. */
int rv_verify_partition(int world, int rank, uint8_t groups[32], uint32_t *n_groups);
/* COLLECTIVE: every rank passes the same proof bytes and flags, and *ok is rv_verify_ex's answer on EVERY rank.  The format and
 * record checks run before the all-gather, so a malformed proof gets the same return code and *ok on every rank and no rank
 * waits for another; so does a communicator whose world does not divide 32 (RV_E_ARG).  world == 1: a device copy instead of
 * RCCL.  c must have been compiled on the rank's own context. */
int rv_verify_sharded(rv_comm *comm, const rv_circuit *c, const uint8_t *proof, size_t proof_len, uint32_t flags, int *ok);
/* One process, n GPUs: a host thread per rank runs rv_verify_sharded; returns the ranks' common (rc, *ok) -- ranks that
 * disagree (which the design rules out) give RV_E_DEVICE with rv_last_error naming them */
int rv_verify_multi(rv_comm *const *comms, const rv_circuit *const *circuits, int n, const uint8_t *proof, size_t proof_len,
                    uint32_t flags, int *ok);

/* Many proofs of one circuit in one pass (the verifier's counterpart of rv_prove_batch; GF(2), Z64 and mixed circuits below
 * the large-circuit threshold -- larger ones verify proof after proof): ok[b] as rv_verify_ex would set it for
 * proofs[b] with the same flags.  A proof whose bytes cannot be parsed (or whose records rv_verify_ex would answer with
 * RV_E_PROOF_MALFORMED) is a REJECTED proof, ok[b] = 0, and the others are verified all the same; a non-zero return
 * code means an argument or device error. */
int rv_verify_batch(rv_ctx *ctx, const rv_circuit *c, size_t batch, const uint8_t *const *proofs, const size_t *proof_lens,
                    uint32_t flags, int *ok /* [batch] */);

/* rv_verify_batch on proofs that lie in device memory: d_proofs is a HOST array of device pointers, d_proofs[b] to
 * proof_lens[b] bytes of bincode(Proof) (what rv_prove_batch_device wrote, or any bytes).  DEFINITION: the return code and
 * every ok[b] are exactly those of rv_verify_batch on host copies of the same byte strings, for every byte string.
 * Every d_proofs[b] must be memory of the context's device, 16-byte aligned, with proof_lens[b] inside its allocation:
 * RV_E_ARG otherwise, before any kernel runs.  One kernel walks every proof's framing; a proof whose walk stops (bytes that run
 * out, wrong repetition counts, records the verifier's slots cannot take) is copied to the host, where the host verifier's
 * own parse answers it; the others are verified where they lie and no byte of them crosses to the host -- in one pass
 * (chunked by free memory and RV_BATCH_MAX as rv_verify_batch), or through rv_verify_device's path one after another for
 * fewer than two such proofs, a batch of one, or a circuit from RV_BATCH_BIG_GATES on. */
int rv_verify_batch_device(rv_ctx *ctx, const rv_circuit *c, size_t batch, const uint8_t *const *d_proofs /* host array of device pointers */,
                           const size_t *proof_lens, uint32_t flags, int *ok /* [batch] */);

/* ---- Bristol front end (host only, no GPU) ---------------------------------------------
 * The reference's README promises Bristol-format circuits; the parser itself lives in the
 * un-vendored `mcircuit` crate.  This turns Bristol text into the rv_op stream:
 *   wires 0..n_in-1            -> GF2 Input(w), in wire order (= witness order)
 *   XOR -> Add, AND -> Mul, INV / NOT -> AddConst(.., 1), EQW -> AddConst(.., 0), EQ -> Const,
 *   MAND -> one Mul per lane
 *   if expected_outputs != NULL: for each output wire (the last n_out wires, in order)
 *   AddConst(tmp, w, expected) + AssertZero(tmp)  — the statement "the circuit maps the witness
 *   to these outputs" (SURVEY §8d configs 1-3); n_expected must equal the circuit's output count (RV_E_ARG otherwise,
 *   before anything is read from expected_outputs).
 * format: 0 = auto, 1 = Bristol Fashion ("ngates nwires / niv n.. / nov n.."), 2 = old Bristol
 * ("ngates nwires / n1 n2 n3").  ops is library-allocated (rv_free). */
typedef struct rv_bristol_info {
    uint64_t n_gates, n_wires, n_inputs, n_outputs;
    uint64_t n_and, n_xor, n_inv, n_other;
    uint64_t gf2_wires; /* wire count to pass to rv_circuit_compile (includes assertion temporaries) */
} rv_bristol_info;
int rv_bristol_parse(const char *text, size_t len, int format, const uint8_t *expected_outputs, size_t n_expected, rv_op **ops,
                     size_t *n_ops, rv_bristol_info *info);
/* host only, no GPU: the header lines alone, by the code rv_bristol_parse runs on them -- line 1, the Fashion / old-Bristol decision
 * (for the ambiguous "2 a b" second line a look at the first gate line), the input and output counts, and the checks that need no
 * gate: n_inputs > n_wires and n_outputs > n_wires (RV_E_WIRE_OOB), n_gates > len / 8 + 1 (RV_E_BAD_OP).  info receives n_gates,
 * n_wires, n_inputs and n_outputs, its other fields 0; *gates_offset the offset of the byte behind the last header line, where the gate
 * lines begin.  The return code is rv_bristol_parse's for the same header defect; gate lines do not concern it.  text[0, len) must
 * reach the end of the first non-blank gate line (the look-ahead reads it), and len enters the n_gates check: pass the whole text
 * where it is at hand.  RV_E_ARG: a null argument. */
int rv_bristol_header(const char *text, size_t len, int format, rv_bristol_info *info, size_t *gates_offset);
/* rv_bristol_parse on the context's GPU: d_ops receives exactly the records rv_bristol_parse returns for the same bytes
 * and arguments, byte for byte (the leading Input ops, one Mul per MAND lane, the assertion pairs, zeroed reserved and padding bytes),
 * *n_ops and *info the same counts, and the return code is rv_bristol_parse's for every byte string: that of the first bad gate line
 * in line order, decided inside the line in the host parser's order.  On an error *n_ops is 0 and d_ops holds anything.
 * text: text_on_device == 0, host memory, copied by the library into context-arena memory; otherwise memory of the context's device
 * (no alignment asked; inside one allocation where the runtime can tell, RV_E_ARG otherwise, before anything is launched) -- the
 * library copies down only the first bytes that hold four non-blank lines, for the header code.  expected_outputs is host memory.
 * d_ops / cap_ops: cap_ops records in the memory of the context's device, rv_circuit_compile_device's conventions (8-byte aligned,
 * inside one allocation; the caller keeps it).  d_ops == NULL or cap_ops < the record count: RV_E_ARG with *n_ops = the count and info
 * filled, nothing written (rv_stream_finish_device's rule) -- so a sizing call (NULL, 0) validates the whole text, and returns the
 * text's own code when it has one.  No allocation follows the header's claims: a few bytes may name 2^32 - 1 inputs, and the count
 * is merely reported.  Order of decisions: arguments (RV_E_ARG); len >= 2^32 (RV_E_UNSUPPORTED); the header's code (RV_E_ARG for
 * n_expected != n_outputs among them); the gate lines' code; more than 2^32 - 1 wires with the assertion temporaries
 * (RV_E_UNSUPPORTED); capacity; the records.
 * Work memory comes from the context arena and goes back before the call returns: 8 bytes per gate line the header names (at most
 * len / 8 + 1 lines: about one byte per byte of text at the very most, a third of that for ordinary lines), 8 bytes per 4096 bytes
 * of text, and the text itself (and n_expected bytes) when it comes from host memory.  Runs on the context's stream and
 * synchronises it once, at the end (a device text: once more for the header bytes). */
int rv_bristol_parse_device(rv_ctx *ctx, const char *text, size_t len, int text_on_device, int format, const uint8_t *expected_outputs /* host */,
                            size_t n_expected, rv_op *d_ops, size_t cap_ops, size_t *n_ops, rv_bristol_info *info);
/* the device parser's two tile sizes: out[0] = bytes of text per workgroup of the tile kernels, out[1] = gate lines per workgroup of
 * the line kernels (the lengths the tests go around) */
int rv_hook_bristol_tiles(uint32_t out[2]);
/* host only, no GPU: rv_bristol_header for the HEAD of a text -- text[0, len) is a prefix (it must reach the end of the first non-blank
 * gate line, or be the whole text) of a text of full_len bytes, and full_len, not len, enters the n_gates > full_len / 8 + 1 check.
 * With len == full_len this is rv_bristol_header.  RV_E_ARG: a null argument, or len > full_len. */
int rv_bristol_header_prefix(const char *text, size_t len, uint64_t full_len, int format, rv_bristol_info *info, size_t *gates_offset);

/* ---- a Bristol text read in windows ---------------------------------------------
 * rv_bristol_parse_device for a text that is handed over in consecutive byte ranges ("feeds") of any length, 0 and 1 included:
 *     rv_bristol_reader_begin(ctx, file_len, format, expected, n_expected, &r)
 *     rv_bristol_reader_feed(r, text, len, on_device, d_ops, cap_ops, &piece)      the next len bytes of the text, again and again
 *     rv_bristol_reader_finish(r, &info)
 *     rv_bristol_reader_destroy(r)
 * Over all feeds the records delivered, in order, are rv_bristol_parse's records for the whole text and the same arguments, byte for
 * byte; the first nonzero code a feed returns is its code; finish fills info as it does -- for every byte string the host parser
 * answers and every way of cutting it.  file_len may be 2^32 and more; one feed stays below 2^32 bytes.
 *   The header: the reader keeps the first bytes on the host until they hold four whole non-blank lines or the file ends (of a device
 * text it copies down only those: 4096 bytes, then as many again as it holds), and runs rv_bristol_parse's header code on them with
 * the file's length.  That feed returns the header's code (RV_E_ARG for n_expected != n_outputs among them) and its piece begins with
 * the n_inputs Input records.
 *   The lines: a gate line is final when its LF has been fed or the bytes fed reach file_len.  A feed judges and delivers exactly the
 * final lines not yet delivered whose index is below n_gates; an unfinished line is never judged, so a bad line's code is returned by
 * the feed that makes it final (among several the first in line order counts).  The feed that makes line n_gates - 1 final ends its
 * piece with the assertion pairs (n_gates == 0: the header feed) and returns RV_E_UNSUPPORTED, after its lines' own codes, for more
 * than 2^32 - 1 wires with the assertion temporaries.  Bytes behind that line are never judged and need not be fed.  A file that ends
 * with fewer lines: RV_E_BAD_OP from the feed that reaches file_len.
 *   After a code of the text the reader accepts only destroy (RV_E_ARG otherwise); what earlier feeds delivered is then anything.
 * finish: RV_OK once the header is in and n_gates lines and the pairs are out, RV_E_ARG before.
 *   d_ops / cap_ops: rv_bristol_parse_device's conventions.  cap_ops below what the feed delivers: RV_E_ARG with piece->n_ops = the
 * count needed, nothing written and the reader unchanged -- the same bytes are fed again with a larger buffer.  This many always
 * suffice: the Input records still due + (held + len) / 6 + 1 + 2 * n_expected, where `held` is what was fed before and no feed
 * has made final -- the bytes behind the last LF fed, and every byte fed while the header is not complete.  (A MAND lane, three
 * numbers and their blanks, takes six bytes of a line; any other record a line of eleven at least.)  d_ops == NULL is a scan feed:
 * nothing is written, the piece and the info are complete; scan feeds and writing feeds mix.
 *   RV_E_ARG with the reader unchanged, before any launch: a NULL r or piece, NULL text with len != 0, len >= 2^32, a feed past
 * file_len, d_ops misaligned or outside an allocation, a device text outside an allocation.  held + len >= 2^32: RV_E_UNSUPPORTED,
 * the reader unchanged.  No byte outside text[0, len) is read.
 *   Memory: the unfinished last line (the carry) lives in context-arena memory between feeds; a line may span any number of feeds.
 * A feed's work memory -- the carry and the window in one buffer, 8 bytes per 8 bytes of it for the line table at the most, 8 bytes
 * per 4096 for the tiles -- is sized by carry + len, never by file_len, n_gates or n_inputs, and goes back before the feed returns.
 * A feed runs on the context's stream and synchronises it twice (the header feed of a device text once more per copy of header
 * bytes), whatever len is. */
typedef struct rv_bristol_reader rv_bristol_reader;
typedef struct rv_bristol_piece {
    uint64_t first_op, n_ops;     /* records this feed delivered: ordinals in rv_bristol_parse's list */
    uint64_t n_input_gf2;         /* Input ops among them */
    uint64_t first_line, n_lines; /* gate lines this feed made final */
} rv_bristol_piece;               /* 40 bytes */
int rv_bristol_reader_begin(rv_ctx *ctx, uint64_t file_len, int format, const uint8_t *expected_outputs /* host, copied; may be NULL */,
                            size_t n_expected, rv_bristol_reader **out);
int rv_bristol_reader_feed(rv_bristol_reader *r, const char *text, size_t len, int text_on_device, rv_op *d_ops, size_t cap_ops,
                           rv_bristol_piece *piece);
/* RV_E_ARG until the header is in; then n_gates, n_wires, n_inputs, n_outputs and gf2_wires (the class counts: of the lines so far) */
int rv_bristol_reader_header(rv_bristol_reader *r, rv_bristol_info *info);
int rv_bristol_reader_finish(rv_bristol_reader *r, rv_bristol_info *info /* may be NULL */);
void rv_bristol_reader_destroy(rv_bristol_reader *r);
/* tests only, as rv_hook_program_reader_resume: the reader continues at byte file_off of the file, with gate line next_line and
 * record next_op, nothing carried and the Input records out.  The header: that of a first feed of the header lines alone. */
int rv_hook_bristol_reader_resume(rv_bristol_reader *r, uint64_t file_off, uint64_t next_line, uint64_t next_op);

/* ---- wire indices compacted by liveness -----------------------------------------
 * A stream's wire store is sized by the wire counts it begins with: one row per wire index.  An op list in SSA form (a Bristol file,
 * a list a parallel generator wrote) names one index per gate.  These two calls renumber the wires of a whole op list so that an
 * index is reused once the value on it has had its last reader.  The proof does not depend on wire numbering (masks and transcript
 * events follow op order), so the proof of the renumbered list under its new counts is byte for byte the proof of the original.
 *
 * The rule: every op with a destination defines a value; a read refers to the last value defined on its index.  The GF(2) indices
 * inside any B2A range [a, a + 63] are pinned: they map to their rank among the pinned indices (new indices 0 .. P - 1, consecutive
 * ranges stay consecutive) and are never reused.  A read of a non-pinned index that no earlier op wrote maps to one reserved,
 * never-written wire of its domain (new GF(2) index P, new Z64 index 0; reserved only if there is such a read).  Every other value
 * takes a slot from its domain's FIFO pool behind these, per op in this order: the destination takes the head of the queue (a fresh
 * slot when it is empty); then each operand value whose last reader is this op is released to the tail (a before b; once when both
 * name it); then the op's own value, if nothing reads it.  SizeHint ops stay in place with the new counts as their fields, so op
 * indices keep their meaning and no count grows.  Input ops keep their places: witness order is unchanged.  RV_COMPILE_KEEP_WIRES and
 * rv_evaluate* wire values refer to the new indices: the renumbered dst of an op is where its value lives.
 *
 * The slot count is the largest number of values alive across one op; for a list that is already tight the new count can exceed the
 * old by one (the destination is allocated before the operands are released) plus the zero wire.  info reports the counts; whether to
 * use the new list is the caller's choice.  info may be NULL.
 *
 * Errors: the list is validated as rv_circuit_compile validates it (domain, opcode, reserved, every wire index against the count in
 * force at its op) and the code is the one rv_circuit_compile returns for the list -- that of the first bad op in op order.  Nothing
 * is written then.  out may equal ops (in place); any other overlap is RV_E_ARG. */
typedef struct rv_compact_info {
    uint64_t z64_wires, gf2_wires;         /* new counts */
    uint64_t gf2_pinned;                   /* P */
    uint32_t gf2_zero_wire, z64_zero_wire; /* 1 if reserved */
    uint64_t gf2_values, z64_values;       /* values defined */
} rv_compact_info;
/* host only, no GPU (like rv_bristol_parse): the sequential sweep */
int rv_ops_compact_wires(const rv_op *ops, size_t n_ops, size_t z64_wires, size_t gf2_wires, rv_op *out, rv_compact_info *info);
/* The same result from kernels on the context's GPU, for a list that lies in device memory: d_ops and d_out are n_ops packed records
 * in the memory of the context's device (rv_circuit_compile_device's conventions: the caller keeps ownership and must have finished
 * writing d_ops; 8-byte aligned and inside an allocation of that device, RV_E_ARG otherwise, before anything is launched); d_out may
 * equal d_ops.  Work memory (about 70 bytes per op, 8 per GF(2) wire index when the list has B2A ops) comes from the context arena
 * and goes back before the call returns.  RV_E_UNSUPPORTED: 2^31 ops or more, or a wire count in force of 2^31 or more. */
int rv_ops_compact_wires_device(rv_ctx *ctx, const rv_op *d_ops, size_t n_ops, size_t z64_wires, size_t gf2_wires, rv_op *d_out,
                                rv_compact_info *info);

/* The same result for a list that is read in windows: the list passes through in feeds, twice -- a scan pass, then a
 * rewrite pass -- and the records of all rewrite feeds together are rv_ops_compact_wires' records byte for byte, `info` its info,
 * however the two passes are cut (the cuts are independent; feeds of 0 and 1 ops are allowed).
 *
 *   begin -> scan* -> scan_end [-> scan* -> scan_end] -> feed* [-> rewind -> feed*]... -> destroy
 *
 * scan       validates the ops (against the counts in force, carried from feed to feed) and records liveness.  A list
 *            rv_ops_compact_wires refuses is refused with the same code by the scan feed that holds the first bad op in op order;
 *            after that only destroy is accepted.
 * scan_end   *again = 1: the list holds a B2A op.  Which GF(2) indices are pinned is known only now, and pinning changes which ops
 *            take slots, so the whole list must be scanned once more (nothing is validated a second time), and scan_end called
 *            again; it then gives *again = 0.  *again = 0: info is filled (when not NULL) and the rewrite pass may begin.
 * feed       writes the feed's n_ops renumbered records to d_out (device memory; may equal a device `ops`, no other overlap).
 * rewind     after a complete rewrite pass: the next feed is op 0 again (a prover reads its source twice).
 *
 * ops: host memory (ops_on_device == 0; the library uploads the feed) or memory of the context's device, by
 * rv_circuit_compile_device's conventions, checked before anything is launched.  A rescan and every rewrite pass must be the list of
 * the first scan: each pass carries the position-keyed digest of its ops and their count; a feed beyond the first scan's count, a
 * scan_end or rewind of a shorter pass, and a digest that differs at the end of a pass (reported by the last feed of a rewrite pass,
 * by scan_end of a rescan) are RV_E_ARG.  Calling out of order is RV_E_ARG and leaves the object as it was.  RV_E_UNSUPPORTED: 2^31
 * ops or more in all (from the feed that crosses it) or in one feed, a wire count in force of 2^31 or more.
 * RV_E_NOMEM or RV_E_DEVICE from any call: the carried state may be half moved; only destroy is accepted afterwards.
 *
 * Memory, all from the context arena.  Held between calls (rv_compactor_info.state_bytes, at most
 *   8 * (Wz + Wg) + 8 * Wg * [a B2A op was met] + total_ops + 4 * (new z64 count + new gf2 count) + 4096):
 *   8 bytes per wire index in force per domain (the tables grow when a SizeHint raises a count), 8 more per GF(2) index once a B2A op
 *   was met (pinned flags and ranks), one mark byte per op of the list, 4 bytes per new slot (the free-slot queues).  Nothing else
 *   follows the list's length; the index tables follow the OLD wire counts, which is what liveness needs to know.
 * Per feed, given back before the call returns (peak_feed_bytes: the largest so far): 20 bytes per op of the feed in a scan feed, 68 in
 *   a rewrite feed, plus 24 per op for an uploaded host feed and the scans' block sums (below 1 %).  scan_end reads the marks once,
 *   with 24 bytes per 256 ops. */
typedef struct rv_compactor rv_compactor;
typedef struct rv_compactor_info {
    uint64_t total_ops;       /* ops of the first scan pass so far (the list's length once it ended) */
    uint64_t state_bytes;     /* device memory held now */
    uint64_t peak_feed_bytes; /* the most work memory one call took */
    uint32_t scans;           /* scan passes ended */
    uint32_t b2a;             /* 1: a B2A op was met */
} rv_compactor_info;
int rv_compactor_begin(rv_ctx *ctx, size_t z64_wires, size_t gf2_wires, rv_compactor **out);
int rv_compactor_scan(rv_compactor *c, const rv_op *ops, size_t n_ops, int ops_on_device);
int rv_compactor_scan_end(rv_compactor *c, int *again, rv_compact_info *info /* filled when *again == 0; may be NULL */);
int rv_compactor_feed(rv_compactor *c, const rv_op *ops, size_t n_ops, int ops_on_device, rv_op *d_out);
int rv_compactor_rewind(rv_compactor *c);
int rv_compactor_get_info(const rv_compactor *c, rv_compactor_info *info);
void rv_compactor_destroy(rv_compactor *c);

/* ---- program files (host only, no GPU) ---------------------------------------------------
 * The reference CLI reads its gate stream as bincode 1.3 of Vec<mcircuit::CombineOperation>
 * (src/main.rs:66,98,122).  rv_program_from_bincode turns such a file into rv_op records, rv_program_to_bincode
 * writes one.  The enum's variant order comes from the un-vendored `mcircuit` crate and is the one SURVEY A.7
 * recalls (GF2, Z64, B2A, SizeHint; Input, Random, Add, AddConst, Sub, SubConst, Mul, MulConst, AssertZero, Const):
 * it cannot be verified here, so nothing selects this format automatically.  Wire indices above 2^32-1 ->
 * RV_E_UNSUPPORTED; a truncated file, an unknown variant or a bool that is not 0/1 -> RV_E_BAD_OP.  Outputs are
 * library-allocated (rv_free). */
int rv_program_from_bincode(const uint8_t *data, size_t len, rv_op **ops, size_t *n_ops);
int rv_program_to_bincode(const rv_op *ops, size_t n_ops, uint8_t **data, size_t *len);
/* The same two on the context's GPU: a program file read into, and written from, op records in device memory.  The
 * host pair above stays the definition and needs no GPU; the record layout both device calls read is one table
 * (csrc/bincode_dev.h), with the variant order recalled above -- so nothing selects this format automatically here either. */
typedef struct rv_program_info {
    uint64_t n_ops;                /* the vector's length */
    uint64_t bytes;                /* offset behind the last record read: bytes after it were not looked at */
    uint64_t z64_wires, gf2_wires; /* mcircuit::largest_wires: what reverie_amd.ops.largest_wires returns for the records */
    uint64_t n_gf2, n_z64, n_b2a, n_sizehint;
} rv_program_info;
/* rv_program_from_bincode for bytes the GPU parses: d_ops receives exactly the records rv_program_from_bincode returns for the same
 * bytes, byte for byte (reserved and unused fields zero), *n_ops the same count, and the return code is rv_program_from_bincode's
 * for every byte string: len < 8 or a count above (len - 8) / 16 is RV_E_BAD_OP (nothing is allocated or launched by what the count
 * claims); then the code of the first of the `count` records that has one, decided inside the record in the host's order (an unknown
 * domain or opcode, a bool above 1, a record that does not end inside len: RV_E_BAD_OP; else a wire field above 2^32 - 1:
 * RV_E_UNSUPPORTED); fewer than `count` records before len: RV_E_BAD_OP.  Bytes behind record count - 1 are never judged.  A count of 0
 * is RV_OK, nothing is written and no capacity is asked for.  On an error *n_ops is 0 and d_ops holds anything.
 * data: data_on_device == 0, host memory, copied by the library into context-arena memory; otherwise memory of the context's device
 * (no alignment asked; inside one allocation where the runtime can tell, RV_E_ARG otherwise, before anything is launched).  No byte
 * outside data[0, len) is read.  d_ops / cap_ops: rv_circuit_compile_device's conventions (8-byte aligned, inside one allocation of
 * the context's device; the caller keeps it).  d_ops == NULL or cap_ops < count: RV_E_ARG with *n_ops = the count and info filled,
 * nothing written -- after the whole input has been validated: a sizing call (NULL, 0) on bad bytes returns the bytes' own code.
 * Order of decisions: arguments (RV_E_ARG); len >= 2^32 (RV_E_UNSUPPORTED); the header; the records; capacity; writing.  info may
 * be NULL.
 * Work memory comes from the context arena and goes back before the call returns: 72 bytes per 4096 bytes of data (the tiles' entry
 * maps: 1.8 % of len), 264 bytes per 2^20 bytes, some 3 KiB of counters, and the data itself when it comes from host memory.  Runs on
 * the context's stream and synchronises it once, at the end (device data: once more for the 8 header bytes). */
int rv_program_from_bincode_device(rv_ctx *ctx, const uint8_t *data, size_t len, int data_on_device, rv_op *d_ops, size_t cap_ops,
                                   size_t *n_ops, rv_program_info *info /* may be NULL */);
/* rv_program_to_bincode for records in device memory: d_out receives the bytes rv_program_to_bincode writes for the same records
 * (GF(2) immediates as imm & 1), and the return code is its code: reserved != 0, an unknown domain or opcode -> RV_E_BAD_OP.
 * d_ops as above (n_ops records); d_out / cap: memory of the context's device, no alignment asked.  d_out == NULL or cap < the
 * file's length: RV_E_ARG with *len = the length, nothing written.  A file of 2^32 bytes or more: RV_E_UNSUPPORTED.  Work memory
 * (4 bytes per record) comes from the context arena and goes back before the call returns; one synchronisation of the context's
 * stream, at the end. */
int rv_program_to_bincode_device(rv_ctx *ctx, const rv_op *d_ops, size_t n_ops, uint8_t *d_out, size_t cap, size_t *len);
/* out[0] = bytes of the file per tile of the walk and decode kernels, tiles counted from data[0] whatever its address; out[1] =
 * tiles per workgroup of the composing scan (the lengths the tests go around) */
int rv_hook_bincode_tiles(uint32_t out[2]);

/* A program file read in windows: rv_program_from_bincode_device for a file that is handed over in consecutive byte
 * ranges of any length (0 and 1 included; one range below 2^32 bytes), so that neither the file nor its records are ever whole in
 * memory.  file_len may be 2^32 and more.
 *     rv_program_reader_begin(ctx, file_len, &r)
 *     rv_program_reader_feed(r, data, len, on_device, d_ops, cap_ops, &piece)      the next len bytes of the file, again and again
 *     rv_program_reader_finish(r, &info)
 *     rv_program_reader_destroy(r)
 * DEFINITION, for every byte string and every way of cutting it: the records delivered over all feeds, in order, are the records
 * rv_program_from_bincode returns for the whole file, byte for byte, and the first nonzero code a feed (or finish) returns is its
 * code.  A feed delivers to d_ops[0, piece->n_ops) the records not yet delivered whose last byte lies in the bytes fed so far and
 * whose ordinal is below the header's count; no byte outside data[0, len) is read.  file_len < 8 (at the first feed) or a count above
 * (file_len - 8) / 16 (as soon as the 8 header bytes are in; nothing is sized by the count) is RV_E_BAD_OP; a record's own code is
 * bc_decode's (RV_E_BAD_OP before RV_E_UNSUPPORTED); a position no record can be read at is RV_E_BAD_OP once 32 bytes lie behind it
 * or the file ends; so is the end of the file below the count.  After such a code the reader accepts only destroy (RV_E_ARG), and
 * what earlier feeds delivered is "anything".  Bytes behind record count - 1 are never judged and need not be fed: finish is RV_OK
 * with the whole file's info (bytes: the 64-bit file offset behind record count - 1) once `count` records are out (a count of 0:
 * once the header is in), RV_E_ARG before.
 * Arguments (RV_E_ARG, the reader's state unchanged): r, piece or (with len) data NULL; len >= 2^32 (before data is looked at);
 * feeding past file_len; a non-NULL d_ops with cap_ops < len / 16 + 1 (the records inside the feed plus one that straddles in:
 * always enough), before anything is launched.  d_ops == NULL is a scan feed: nothing is written, the piece and the info are
 * complete; scan feeds and writing feeds mix.  data / d_ops: rv_program_from_bincode_device's conventions (host data is uploaded by
 * the library; device data needs no alignment).
 * Work memory comes from the context arena by len, never by file_len or the count, and goes back before the feed returns.  A feed
 * runs on the context's stream and ends with one synchronisation (device data: once more for the feeds that bring the 8 header
 * bytes). */
typedef struct rv_program_reader rv_program_reader;
typedef struct rv_program_piece {
    uint64_t first_op, n_ops;          /* the records this feed delivered: ordinals first_op .. first_op + n_ops - 1 */
    uint64_t n_input_gf2, n_input_z64; /* Input ops among them = what a stream feed of these records takes from the witness */
} rv_program_piece;
int rv_program_reader_begin(rv_ctx *ctx, uint64_t file_len, rv_program_reader **out);
int rv_program_reader_feed(rv_program_reader *r, const uint8_t *data, size_t len, int data_on_device, rv_op *d_ops, size_t cap_ops,
                           rv_program_piece *piece);
int rv_program_reader_finish(rv_program_reader *r, rv_program_info *info /* may be NULL */);
void rv_program_reader_destroy(rv_program_reader *r);
/* Tests only: places a fresh reader as if file_off bytes holding next_op whole records had been read, with an empty carry (offsets
 * and ordinals above 2^32 without 4 GB of input).  The count stays open: every whole record is delivered, and finish closes it at
 * the records delivered, where the bytes fed end with a record. */
int rv_hook_program_reader_resume(rv_program_reader *r, uint64_t file_off, uint64_t next_op);

/* ---- Bristol text and program files written on the GPU, whole and in windows --------------------
 * rv_bristol_write (host only, no GPU) is the definition: the records as Bristol Fashion text, exactly what reverie_amd.bristol.dumps
 * returns for them.  The header is "%d %d\n1 %d\n1 %d\n\n" of the gate count, n_wires, the input count and n_outputs; the input count
 * is the length of the leading run of GF(2) Input records, the gate count the records behind it.  Each later record is one line:
 * Add "2 1 a b dst XOR", Mul "2 1 a b dst AND", AddConst 1 "1 1 a dst INV", AddConst 0 "1 1 a dst EQW", Const "1 1 imm dst EQ";
 * the fields a line does not name are ignored.  n_wires == 0: the count is the largest index named plus one, or the input count if
 * that is larger.  text is library-allocated (rv_free).
 *   RV_E_ARG, before anything else: NULL text or len, or NULL ops with n_ops != 0.  Then the code of the first record in list order
 * that has one; inside a record: (1) reserved != 0, an unknown domain or opcode (rv_program_to_bincode's rule): RV_E_BAD_OP; (2) a
 * valid record Bristol text cannot say -- a domain other than GF(2), an Input behind the leading run, an Input of the run whose dst is
 * not its position, Random, Sub, SubConst, MulConst or AssertZero, AddConst or Const with imm > 1: RV_E_UNSUPPORTED; (3) with a stated
 * n_wires, an index the line names that is >= n_wires: RV_E_WIRE_OOB (an Input record has no line: the input count is checked next).
 * Behind the records: n_outputs > n_wires or the input count > n_wires: RV_E_WIRE_OOB (rv_bristol_parse's header checks). */
int rv_bristol_write(const rv_op *ops, size_t n_ops, uint64_t n_wires /* 0: derive */, uint64_t n_outputs, char **text, size_t *len);
/* rv_bristol_write for records in device memory: d_text receives the bytes rv_bristol_write produces and the return code is its code,
 * for every record list.  d_ops: n_ops records, rv_circuit_compile_device's conventions (8-byte aligned, inside one allocation of the
 * context's device); d_text / cap: memory of that device, no alignment asked.  d_text == NULL or cap < the text's length: RV_E_ARG
 * with *len = the length, nothing written -- after the records have been judged, so a sizing call (NULL, 0) on bad records returns
 * their code.  A text of 2^32 bytes or more, or 2^32 records or more: RV_E_UNSUPPORTED.  Nothing is written for a list with a code.
 * Work memory (4 bytes per record plus the scan's sums, 8 bytes per 2048 records) comes from the context arena and goes back before
 * the call returns; the call runs on the context's stream and synchronises it once, at the end. */
int rv_bristol_write_device(rv_ctx *ctx, const rv_op *d_ops, size_t n_ops, uint64_t n_wires, uint64_t n_outputs, char *d_text, size_t cap,
                            size_t *len);
/* out[0] = records per workgroup of the emit kernel, out[1] = records per workgroup of the scan (the sizes the tests go around) */
int rv_hook_bristol_write_tiles(uint32_t out[2]);

/* The two writers fed in windows: consecutive pieces of a record list ("feeds") of any length, 0 and 1 included.
 *     rv_bristol_writer_begin(ctx, n_ops, n_inputs, n_wires, n_outputs, &w)      rv_program_writer_begin(ctx, n_ops, &w)
 *     rv_bristol_writer_feed(w, ops, n, ops_on_device, d_text, cap, &piece)      rv_program_writer_feed(w, ops, n, ops_on_device, d_out, cap, &piece)
 *     rv_bristol_writer_finish(w)                                                rv_program_writer_finish(w)
 *     rv_bristol_writer_destroy(w)                                               rv_program_writer_destroy(w)
 * DEFINITION, for every record list and every way of cutting it: the bytes of all feeds, in order, are the bytes of
 * rv_bristol_write(ops, n_ops, n_wires, n_outputs), respectively rv_program_to_bincode(ops, n_ops), on the whole list, and the first
 * nonzero code a feed returns is that call's code.  The first feed's bytes begin with the header (the Bristol header lines, or the
 * 8-byte count), whatever the feed's length; a record is written whole by the feed that brings it; nothing is carried between feeds
 * but the next ordinal, the file offset and "the header is out", and memory follows the feed, never the list.  n_ops and file_off may
 * be 2^32 and more; one feed's bytes stay below 2^32 (RV_E_UNSUPPORTED, the writer unchanged; so is a Bristol feed of 2^32 records
 * and a program feed of 2^28 records or more).
 *   The Bristol writer is told at begin what the whole-list call derives, because the header goes out first: record i < n_inputs must
 * be GF(2) Input(i), a record at or behind n_inputs must not be an Input (RV_E_UNSUPPORTED at that record, in rv_bristol_write's order
 * inside the record), and every index a line names is checked against n_wires (RV_E_WIRE_OOB).  begin: RV_E_ARG for n_inputs > n_ops
 * or n_wires == 0 with n_ops != 0, then RV_E_WIRE_OOB for n_inputs or n_outputs above n_wires.  With the values rv_bristol_write
 * would derive the bytes are its bytes.
 *   cap below what the feed writes (or a NULL buffer: a sizing feed): RV_E_ARG with piece->bytes = the need, nothing written and the
 * writer unchanged -- the same records are fed again with a larger buffer.  96 + 41 * n bytes always suffice for Bristol text,
 * 8 + 32 * n for a program file.  Also RV_E_ARG with the writer unchanged, before any launch: a NULL writer or piece, NULL ops with
 * n != 0, feeding past n_ops, device ops misaligned or outside an allocation, a buffer outside an allocation.
 *   After a code of the records the writer accepts only destroy (RV_E_ARG otherwise), and what earlier feeds wrote is "anything".
 * finish: RV_OK once the header and exactly n_ops records are out, RV_E_ARG before.  A list of 0 records is allowed: its header goes
 * out with a feed of 0 records.
 *   ops: host memory (ops_on_device == 0; the library uploads the feed into context-arena memory) or memory of the context's device;
 * host feeds and device feeds mix.  A feed runs on the context's stream and waits for it once; its work memory (4 bytes per record of
 * the feed, the scan's sums, 24 per record of an uploaded feed) goes back before it returns. */
typedef struct rv_bristol_writer rv_bristol_writer;
typedef struct rv_program_writer rv_program_writer;
typedef struct rv_writer_piece {
    uint64_t first_op, n_ops; /* the records of this feed: ordinals first_op .. first_op + n_ops - 1 */
    uint64_t file_off, bytes; /* where the feed's bytes lie in the whole output, and how many they are (or, with RV_E_ARG, would be) */
} rv_writer_piece;
int rv_bristol_writer_begin(rv_ctx *ctx, uint64_t n_ops, uint64_t n_inputs, uint64_t n_wires, uint64_t n_outputs, rv_bristol_writer **out);
int rv_bristol_writer_feed(rv_bristol_writer *w, const rv_op *ops, size_t n, int ops_on_device, char *d_text, size_t cap, rv_writer_piece *piece);
int rv_bristol_writer_finish(rv_bristol_writer *w);
void rv_bristol_writer_destroy(rv_bristol_writer *w);
int rv_program_writer_begin(rv_ctx *ctx, uint64_t n_ops, rv_program_writer **out);
int rv_program_writer_feed(rv_program_writer *w, const rv_op *ops, size_t n, int ops_on_device, uint8_t *d_out, size_t cap, rv_writer_piece *piece);
int rv_program_writer_finish(rv_program_writer *w);
void rv_program_writer_destroy(rv_program_writer *w);

/* ---- witness text read and written on the GPU, whole, in windows and in batches ------------------
 * The witness file of the command line is text that is scanned byte by byte: '0' and '1' are bits, every other byte is skipped.
 * rv_witness_parse (host only, no GPU) is the definition: byte b is a bit iff (b ^ 0x30) <= 1, its value is b & 1, and every byte
 * string is a witness -- the text never produces an error.  bits receives one byte per bit, *n_bits the count.  bits == NULL: the
 * count alone.  cap < the count: RV_E_ARG with *n_bits = the count and nothing written.  RV_E_ARG also for a NULL n_bits, or a NULL
 * text with len != 0. */
int rv_witness_parse(const char *text, size_t len, uint8_t *bits, size_t cap, size_t *n_bits);
/* The writer's definition (host only): bit i becomes '0' + bits[i]; a line feed follows bit i when (i + 1) % line_bits == 0 or
 * i == n - 1 (line_bits == 0: one line).  *len = n + ceil(n / line_bits) (n + 1 with line_bits == 0; 0 for n == 0, the empty text).
 * text == NULL: the length alone (the bits are not looked at).  cap < the length: RV_E_ARG with *len = the length and nothing
 * written.  A byte of bits above 1: RV_E_ARG, the contents of text unspecified.  rv_witness_parse on the text gives the bits back. */
int rv_witness_write(const uint8_t *bits, size_t n, uint64_t line_bits, char *text, size_t cap, size_t *len);
/* rv_witness_parse on the GPU: d_bits[0, *n_bits), the count and the return code are its answers for every byte string and every
 * argument -- count-only with d_bits == NULL, RV_E_ARG with *n_bits = the count when cap is short; then not one byte of d_bits is
 * written (decided on the device: the call runs on the context's stream and synchronises it once, at the end).
 *   text: host memory (text_on_device == 0; uploaded into context-arena memory, and counted as host-to-device witness bytes by
 * rv_hook_witness_traffic) or memory of the context's device, read in place, no alignment asked.  len >= 2^32: RV_E_UNSUPPORTED.
 * d_bits / cap: memory of that device, no alignment asked; it may overlap neither a device text (RV_E_ARG) nor itself.
 *   marks (host, ascending, each <= len, else RV_E_ARG; may be NULL with n_marks == 0): bits_before[m] (host, n_marks) = the number
 * of bits in text[0, marks[m]) -- where each file's bits end when several texts are parsed as one.
 *   Work memory (4 bytes per 4096 bytes of text, the scan's sums, 8 bytes per mark, the text where it is uploaded) comes from the
 * context arena and goes back before the call returns. */
int rv_witness_parse_device(rv_ctx *ctx, const char *text, size_t len, int text_on_device, uint8_t *d_bits, size_t cap, size_t *n_bits,
                            const uint64_t *marks, size_t n_marks, uint64_t *bits_before);
/* out[0] = bytes of text per workgroup of the parse kernels, out[1] = output bytes per workgroup of the writer (the sizes the
 * tests go around) */
int rv_hook_witness_text_tiles(uint32_t out[2]);
/* A text read in windows: consecutive byte ranges ("feeds") of any length, 0 and 1 included, from host memory or from ranges of
 * device memory; host feeds and device feeds mix.  Each feed delivers exactly the bits of its own bytes, so over all feeds the bits
 * are rv_witness_parse's for the whole text, for every way of cutting it.  A text has no records: nothing is carried between feeds,
 * and the reader's state is the two totals finish reports (they may pass 2^32; one feed stays below 2^32 bytes).  A feed is
 * rv_witness_parse_device on its bytes, with its arguments, answers and memory; any answer but RV_OK -- a short cap among them:
 * RV_E_ARG with *n_bits = the count -- leaves the reader unchanged, and the same bytes are fed again.  finish may be called at any
 * time; either pointer may be NULL. */
typedef struct rv_witness_reader rv_witness_reader;
int rv_witness_reader_begin(rv_ctx *ctx, rv_witness_reader **out);
int rv_witness_reader_feed(rv_witness_reader *r, const char *text, size_t len, int text_on_device, uint8_t *d_bits, size_t cap, size_t *n_bits);
int rv_witness_reader_finish(rv_witness_reader *r, uint64_t *bytes_fed, uint64_t *bits_total);
void rv_witness_reader_destroy(rv_witness_reader *r);
/* rv_witness_write on the GPU: d_text receives its bytes and the return code is its code, for every list in device memory (d_bits,
 * d_text / cap: memory of the context's device, no alignment asked, not overlapping).  d_text == NULL: the length alone.  n or the
 * length >= 2^32: RV_E_UNSUPPORTED.  Runs on the context's stream and synchronises it once. */
int rv_witness_write_device(rv_ctx *ctx, const uint8_t *d_bits, size_t n, uint64_t line_bits, char *d_text, size_t cap, size_t *len);

/* ---- programs linked from circuit blocks, on the host and on the GPU, whole and in windows --------
 * A statement is many copies ("instances") of a few function blocks wired together.  rv_link (host only, no GPU) is the definition
 * of the linked op list; the plan below gives its bytes, for any range of ordinals, into device memory.
 *   INPUTS.  blocks[n_blocks]: op lists with their stated wire counts.  A block may hold GF(2), Z64 and B2A records, Random and
 * AssertZero included, and need not be in SSA form.  Its PORTS are its Input records in list order, both domains counted together.
 * block_of[n_instances]: instance i is a copy of blocks[block_of[i]].  bindings[n_bindings]: the bindings of instance i's ports are
 * the entries B(i) .. B(i) + ports(block_of[i]) - 1, B the running sum of the port counts; RV_LINK_WITNESS leaves the port an Input,
 * any other value is a global wire index of the port's domain.  z64_base / gf2_base: the first wire index of instance 0 per domain.
 * head[n_head], tail[n_tail]: op lists in global numbering (constants, global inputs, the assertions on outputs), copied as they are.
 *   OUTPUT: head, the records of instance 0, 1, ... n_instances - 1, tail.  With Z(i) = z64_base + the sum of the stated z64_wires of
 * the blocks of the instances before i, and G(i) likewise, record r of instance i's block is emitted with its domain, opcode,
 * reserved and imm, and Z(i) or G(i) added to every field that names a wire, by the domain of the wire it names: dst in all records
 * but AssertZero; a in all but Input, Random and Const; b in Add, Sub and Mul; in B2A dst is a Z64 wire and a a GF(2) wire.  A field
 * that names no wire is copied unchanged.  An Input whose binding is not RV_LINK_WITNESS becomes AddConst(dst + base, binding, 0) of
 * its domain with b = 0, reserved = 0 and imm = 0: a copy, what the Bristol front end makes of EQW.  Every instance emits exactly its
 * block's record count, so record j of the output is a function of j alone.
 *   INFO, derived without the output: n_ops; n_instances; n_input_gf2 / n_input_z64, the Input records of the whole output;
 * z64_wires / gf2_wires, each the larger of what the largest-index rule (reverie_amd.ops.largest_wires: one more than the largest
 * index a record names, a + 64 for B2A, a SizeHint's own counts) gives for head and tail, and, when there are instances, the base
 * plus the sum of all instances' stated counts.
 *   CODES, the first in this order of decisions:
 *   (1) arguments: a NULL desc or info, a NULL array with a nonzero count, a stated wire count above 2^32: RV_E_ARG; 2^31 instances
 *       or more, or 2^32 block records or more in all: RV_E_UNSUPPORTED;
 *   (2) blocks in order, each block's records in order: reserved != 0, an unknown domain or opcode (rv_program_to_bincode's rule; the
 *       opcode byte of a B2A or SizeHint record is not looked at): RV_E_BAD_OP; a SizeHint: RV_E_UNSUPPORTED; a named index at or above
 *       the stated count of its domain (B2A: dst, and a + 64 above the GF(2) count): RV_E_WIRE_OOB;
 *   (3) head in order, then (4) tail in order: the malformed-record rule (RV_E_BAD_OP) alone; a SizeHint is allowed;
 *   (5) instances in order: block_of[i] >= n_blocks: RV_E_ARG; then n_bindings other than the sum of the port counts: RV_E_ARG; then,
 *       with instances, a base plus the sum of the stated counts that does not fit in 32 bits, and in any case a result wire count
 *       above 2^32 (a B2A of head or tail): RV_E_UNSUPPORTED;
 *   (6) bindings in order: a value other than RV_LINK_WITNESS at or above the result's wire count of its port's domain: RV_E_WIRE_OOB.
 * With a code nothing is returned.  rv_link: *ops is library-allocated (rv_free); ops == NULL gives the info alone. */
#define RV_LINK_WITNESS 0xFFFFFFFFu
typedef struct rv_link_block {
    const rv_op *ops;
    uint64_t n_ops;
    uint64_t z64_wires, gf2_wires; /* the stated counts: the instance's share of the global numbering */
} rv_link_block;
typedef struct rv_link_desc {
    const rv_link_block *blocks;
    uint64_t n_blocks;
    const uint32_t *block_of;
    uint64_t n_instances;
    const uint32_t *bindings;
    uint64_t n_bindings;
    uint64_t z64_base, gf2_base;
    const rv_op *head;
    uint64_t n_head;
    const rv_op *tail;
    uint64_t n_tail;
} rv_link_desc;
typedef struct rv_link_info {
    uint64_t n_ops, n_instances, n_input_gf2, n_input_z64, z64_wires, gf2_wires;
} rv_link_info;
int rv_link(const rv_link_desc *desc, rv_op **ops, rv_link_info *info);
/* The same list from kernels.  A plan is made once per descriptor and then emits any range of ordinals, any number of times and
 * in any order (the streams read a source once per pass):
 *     rv_link_plan_create(ctx, desc, flags, &plan)
 *     rv_link_plan_info(plan, &info)
 *     rv_link_plan_emit(plan, first_op, n, d_ops, &piece)
 *     rv_link_plan_destroy(plan)
 * create: the return code and the info are what rv_link gives for the same descriptor, for every descriptor, and a plan is made
 * only for RV_OK.  The blocks' op lists (RV_LINK_BLOCKS_ON_DEVICE) and block_of / bindings (RV_LINK_TABLES_ON_DEVICE) may lie in the
 * memory of the context's device (rv_circuit_compile_device's conventions: ops 8-byte aligned, tables 4-byte aligned, each inside
 * one allocation; RV_E_ARG otherwise, and for an unknown flag); the rv_link_block array itself, head and tail are host memory.  The
 * plan keeps its own device copy of everything, so nothing of the caller's has to outlive the call.  It runs on the context's stream:
 * every block record is judged (the first code by a 64-bit minimum of position << 8 | code), each block's Input flags are scanned into
 * port ordinals, the instances are scanned into four exclusive 64-bit prefix arrays (op offset, Z, G, B) while block_of is checked,
 * and every binding is checked and counted.  MEMORY held until destroy, from the context arena: the copies (24 bytes per block, head
 * and tail record, 4 per instance and per binding), 4 bytes per block record (port ordinals), 32 bytes per block and 32 per
 * instance (the four prefix arrays).
 * emit: records first_op .. first_op + n - 1 of the output list into d_ops (memory of the context's device, 8-byte aligned, inside
 * one allocation), n == 0 included; piece receives the range and its Input counts per domain, what a stream piece needs.  Ordinals are
 * 64-bit; one call stays below 2^28 records (RV_E_UNSUPPORTED: the program writer's limit).  RV_E_ARG before any launch, with d_ops
 * untouched: a NULL plan or piece, a range outside the list, a NULL (with n != 0), misaligned or foreign d_ops.  The call runs on
 * the context's stream and waits for it once. */
#define RV_LINK_BLOCKS_ON_DEVICE 1u
#define RV_LINK_TABLES_ON_DEVICE 2u
typedef struct rv_link_plan rv_link_plan;
typedef struct rv_link_piece {
    uint64_t first_op, n_ops, n_input_gf2, n_input_z64;
} rv_link_piece;
int rv_link_plan_create(rv_ctx *ctx, const rv_link_desc *desc, uint32_t flags, rv_link_plan **plan);
int rv_link_plan_info(const rv_link_plan *plan, rv_link_info *info);
int rv_link_plan_emit(rv_link_plan *plan, uint64_t first_op, uint64_t n, rv_op *d_ops, rv_link_piece *piece);
void rv_link_plan_destroy(rv_link_plan *plan);
/* out[0] = records per workgroup of the emit kernel, out[1] = items per workgroup of the scans (the sizes the tests go around) */
int rv_hook_link_tiles(uint32_t out[2]);

/* ---- ops no assertion or output depends on, dropped ------------------------------
 * A statement uses part of what its function blocks compute: an AES block of which a few output bytes are asserted, an adder whose
 * sum bits nobody reads, whatever a circuit compiler left behind.  A dead op is not free: a dead Mul is a correction and a broadcast
 * per repetition in the proof, a dead B2A the 442 GF(2) steps it expands into, a dead Random a mask.  These calls drop them.
 *
 * VALUES AND READS are those of the wire compaction above: every op with a destination defines a value on (domain, dst); a read
 * refers to the last value defined on its index before the reading op, and to no value (the zero wire) where no op wrote the index.
 * B2A defines a Z64 value and reads the 64 GF(2) indices a .. a + 63.  Nothing is pinned here: every GF(2) write is a writer like any
 * other, B2A ranges included.
 * ROOTS: every AssertZero; every Input of both domains (witness order and witness length are unchanged); every SizeHint (it stays in
 * place); and, for every index in the caller's two output lists (GF(2) and Z64; both may be empty, an index may repeat), the value
 * that is on that index at the end of the list -- so a function block without assertions can be pruned against its outputs.  An
 * output index no op writes names no value.
 * KEPT: an op is kept if it is a root, or if it defines a value that a kept op reads or that an output names.  Every other op is
 * dropped.  The output is the kept records in list order, byte for byte as they were: nothing is renumbered, the wire counts stay
 * valid as they are.  The kept set is unique (the least set closed under the rule), so the order of work cannot change it; pruning a
 * pruned list with the same outputs changes nothing.  Not done: copy propagation, common subexpressions, dropping unread Inputs
 * (that would change the witness format).  Constant folding is rv_ops_fold below: fold first, then prune.
 *
 * THE PROOF OF A PRUNED LIST IS THE PROOF OF THAT LIST -- byte for byte the reference's proof of the pruned program for the same
 * seeds -- and NOT the proof of the original: unlike the wire compaction this changes proof bytes; that is its purpose.  So prover
 * and verifier both prune, with the same output lists, or the pruned program is the file that is shipped.  Final wire values change
 * as well (RV_COMPILE_KEEP_WIRES, rv_evaluate*): a dropped op's destination keeps whatever was there before.
 *
 * ERRORS: the list is validated as rv_ops_compact_wires validates it and the code is that of the first bad op in op order; then an
 * output index at or above the final wire count of its domain (the stated count, raised by every SizeHint) is RV_E_ARG.  Nothing is
 * written then.
 *
 * THE CALLS: out has room for cap records; *n_out receives the number kept.  out == NULL only counts (*n_out and the info: "what
 * would it save"); cap is not looked at then.  cap below the number kept is RV_E_ARG and nothing is written.  old_index (may be
 * NULL; room for cap entries) receives, for every kept record, the op's index in the old list, so that results such as the first
 * failing AssertZero can be mapped back.  rv_ops_prune may write in place (out == ops; any other overlap is RV_E_ARG).
 * n_out and info may be NULL. */
typedef struct rv_prune_info {
    uint64_t n_kept, n_dropped;
    /* the dropped ops by class */
    uint64_t dropped_gf2_mul, dropped_z64_mul, dropped_b2a, dropped_gf2_random, dropped_z64_random;
    uint64_t dropped_gf2_other, dropped_z64_other; /* Add, AddConst, Sub, SubConst, MulConst, Const */
    /* Inputs that were kept although no kept op reads them and no output names them */
    uint64_t unread_gf2_inputs, unread_z64_inputs;
    uint32_t device_rounds; /* frontier layers the device call peeled (0 from the host call) */
    uint32_t on_device;     /* 1: the device call finished on the GPU (0 from the host call, and from the fall-back) */
} rv_prune_info;            /* 96 bytes */
/* host only, no GPU: the backward sweep -- the definition */
int rv_ops_prune(const rv_op *ops, size_t n_ops, size_t z64_wires, size_t gf2_wires, const uint32_t *outputs_gf2, size_t n_outputs_gf2,
                 const uint32_t *outputs_z64, size_t n_outputs_z64, rv_op *out, size_t cap, size_t *n_out, uint32_t *old_index,
                 rv_prune_info *info);
/* The same records, old_index and info from kernels on the context's GPU, for a list in device memory.  d_ops, d_out (cap records)
 * and d_old_index (cap entries; 4-byte aligned) lie in the memory of the context's device, with rv_ops_compact_wires_device's
 * conventions (8-byte aligned records inside one allocation, RV_E_ARG otherwise and before any launch; 2^31 ops or more, or a wire
 * count in force of 2^31 or more: RV_E_UNSUPPORTED); the two output lists are host memory (they are copied).  ANY overlap of d_out and
 * d_ops is RV_E_ARG before a launch.  Instead of the sweep the kernels count the readers of every value and peel: the first frontier is
 * every value that is no root and has no reader; a round drops each frontier op and takes one from the count of every value it read;
 * values that reach 0 form the next frontier.  Rounds are bounded by the longest chain inside the dead cones, not by the depth of
 * the circuit, and a list with nothing dead costs none.  info->device_rounds counts the frontier layers.  After RV_PRUNE_MAX_ROUNDS
 * layers (environment, read at call time; default 65536) with the frontier not yet empty the call gives up on the device: it copies
 * the list down, runs rv_ops_prune, uploads the result and reports on_device = 0 (device_rounds: the layers peeled until then).
 * The bytes are the same.  Work memory (about 33 bytes per op for a list of one domain, 49 for a mixed one) comes from the context
 * arena and goes back before the call returns.  The call runs on the context's stream and synchronises it. */
int rv_ops_prune_device(rv_ctx *ctx, const rv_op *d_ops, size_t n_ops, size_t z64_wires, size_t gf2_wires, const uint32_t *outputs_gf2,
                        size_t n_outputs_gf2, const uint32_t *outputs_z64, size_t n_outputs_z64, rv_op *d_out, size_t cap, size_t *n_out,
                        uint32_t *d_old_index, rv_prune_info *info);
/* out[0] = threads per workgroup of the peeling kernels, out[1] = the widest frontier one workgroup peels round after round inside
 * one launch (the solo limit), out[2] = rounds between two looks of the host at the device words, out[3] = records per workgroup of
 * the emit kernel, out[4] = RV_PRUNE_MAX_ROUNDS as the next call would read it */
int rv_hook_prune_limits(uint32_t out[5]);
/* launches of this process so far: out[0] = emit kernels that wrote records, out[1] = count-only passes, out[2] = peeling launches
 * (solo and wide together), out[3] = fall-backs to the host sweep */
int rv_hook_prune_launches(uint64_t out[4]);

/* ---- constants folded, record for record ------------------------------------------
 * Real statements wire public values into blocks written for secret ones: the IV and the padding block of a SHA-256, the round keys
 * of a cipher with a public key, a comparison against a public bound, a Z64 factor.  A Mul with a known operand is linear (MulConst)
 * or a constant; a gate whose operands are all known is a Const.  These calls rewrite such records.  The rest of the gain comes from
 * the pruning above, run afterwards: it drops the Consts nothing reads any more.  The order is fold, then prune, then compact.
 *
 * VALUES AND READS are those of rv_ops_prune: every op with a destination defines a value on (domain, dst); a read refers to the last
 * value defined on its index before the reading op, and a read of an index no earlier op wrote reads the zero wire.
 * KNOWN: a value is known, with a value v (GF(2): one bit; Z64: uint64_t with wrapping arithmetic, rv_evaluate's semantics), when
 *   - it is a read of an index no earlier op wrote: known 0;
 *   - Const: known imm (GF(2): bit 0 of imm);
 *   - Add, Sub, Mul with both reads known, AddConst, SubConst, MulConst with their read known: the value the op computes;
 *   - Mul with one read known 0: known 0, whatever the other read is;
 *   - MulConst whose constant is 0 (GF(2): bit 0 of imm is 0): known 0;
 *   - B2A with all 64 reads known: bit k of the value comes from index a + k.
 * Input and Random are never known; AssertZero and SizeHint define nothing.  The known set is the least fixed point of this rule
 * over a DAG in op order, so it is unique whatever the order of work.
 * REWRITE, one to one: record j of the output replaces record j of the input.  Nothing is dropped, moved or renumbered; the op count,
 * the wire counts and the witness order stay.
 *   - a defining op whose value is known becomes Const(dst, v) in the domain of the value (a B2A: a Z64 Const);
 *   - Add(a, b) with exactly one read known becomes AddConst(dst, other, v);
 *   - Sub(a, b) with b known becomes SubConst(dst, a, v); GF(2) Sub(a, b) with a known becomes AddConst(dst, b, v); Z64 Sub(a, b)
 *     with only a known is LEFT AS IT IS (no single op computes c - x);
 *   - Mul(a, b) with exactly one read known, nonzero, becomes MulConst(dst, other, v);
 *   - everything else stays byte for byte as it was: Input, Random, AssertZero, SizeHint, a B2A with an unknown bit, ops with no
 *     known read, and a record that already was a Const (high bits of imm included).
 * A rewritten record has reserved = 0, every field its new opcode does not use set to 0, and a GF(2) imm of 0 or 1.
 * So every wire's final value and every AssertZero's result are the original's for every witness (the difference from pruning);
 * folding a folded list changes nothing; and a list with no Const, no zero MulConst and no read of an unwritten index comes out byte
 * for byte as it went in.
 * NOT DONE: algebraic identities (x + x, x - x, MulConst 1, AddConst 0); copy propagation and common subexpressions; dropping an
 * AssertZero of a known 0 (it is a root and costs nothing in a proof -- the info counts such assertions, and those of a known
 * nonzero value: a statement that can never hold).
 *
 * THE PROOF OF A FOLDED LIST IS THE PROOF OF THAT LIST -- byte for byte the reference's proof of the folded program for the same
 * seeds -- and NOT the proof of the original: a folded Mul or B2A no longer contributes to it.  As with rv_ops_prune, prover and
 * verifier both fold, or the folded program is the file that is shipped.
 *
 * ERRORS: the list is validated as rv_ops_prune validates it; the code is that of the first bad op in op order, and nothing is
 * written then. */
typedef struct rv_fold_info {
    uint64_t n_ops, n_rewritten;
    uint64_t n_known; /* defining ops whose value is known, the Consts already there included */
    /* the rewritten records by class */
    uint64_t gf2_mul_to_const, z64_mul_to_const, gf2_mul_to_linear, z64_mul_to_linear, b2a_to_const;
    uint64_t gf2_other_rewritten, z64_other_rewritten; /* Add / Sub to AddConst / SubConst, a linear op or a zero MulConst to Const */
    /* AssertZeros of a known value (they stay) */
    uint64_t asserts_known_zero, asserts_known_nonzero;
    uint32_t device_rounds; /* layers of known values the device call propagated (0 from the host call) */
    uint32_t on_device;     /* 1: the device call finished on the GPU (0 from the host call, and from the fall-back) */
} rv_fold_info;             /* 104 bytes */
/* host only, no GPU: one forward sweep with a known flag and a value per wire index and domain -- the definition.  out has room
 * for n_ops records; out == NULL only fills the info; out == ops folds in place (any other overlap is RV_E_ARG).  info may be NULL. */
int rv_ops_fold(const rv_op *ops, size_t n_ops, size_t z64_wires, size_t gf2_wires, rv_op *out, rv_fold_info *info);
/* The same records and the same info (but for its last two words) from kernels on the context's GPU, for a list in device memory,
 * with rv_ops_prune_device's conventions (8-byte aligned records inside one allocation of the context's device, RV_E_ARG otherwise
 * and before any launch; 2^31 ops or more, or a wire count in force of 2^31 or more: RV_E_UNSUPPORTED).  d_out == d_ops folds in
 * place (record j is written from record j and the call's own arrays alone); any other overlap is RV_E_ARG.  d_out == NULL counts
 * only.  Instead of the sweep the kernels start from the records that are known at once (Const, a zero MulConst, no written read,
 * a Mul with a zero-wire read) and propagate layer by layer through the readers of every known value; a list with nothing known at
 * once costs no propagation, and one with no unwritten read either is copied.  info->device_rounds counts the layers.  After
 * RV_FOLD_MAX_ROUNDS layers (environment, read at call time; default 65536) with the frontier not yet empty the call gives up on the
 * device: it copies the list down, runs rv_ops_fold, uploads the result and reports on_device = 0.  The bytes are the same.  Work
 * memory comes from the context arena and goes back before the call returns.  The call runs on the context's stream
 * and synchronises it. */
int rv_ops_fold_device(rv_ctx *ctx, const rv_op *d_ops, size_t n_ops, size_t z64_wires, size_t gf2_wires, rv_op *d_out, rv_fold_info *info);
/* out[0] = threads per workgroup of the propagation kernels, out[1] = the widest frontier one workgroup steps layer after layer
 * inside one launch (the solo limit), out[2] = rounds between two looks of the host at the device words, out[3] = records per
 * workgroup of the rewrite kernel, out[4] = RV_FOLD_MAX_ROUNDS as the next call would read it */
int rv_hook_fold_limits(uint32_t out[5]);
/* launches of this process so far: out[0] = rewrite kernels that wrote records, out[1] = count-only passes, out[2] = propagation
 * launches (solo and wide together), out[3] = fall-backs to the host sweep */
int rv_hook_fold_launches(uint64_t out[4]);

/* ---- the same pruning for a list that passes through in windows ------------------
 * rv_pruner_* gives, for a list that arrives in feeds, exactly rv_ops_prune's kept set, records, old_index and class counts, for
 * every list and every way of cutting every pass.  Values, reads, roots and the kept rule are the ones above.  Pruning is a backward
 * data-flow problem, so the MARK pass takes the windows from the last to the first; what one window tells the one before it is one
 * NEEDED byte per wire index and domain (sized by the final wire counts): "a kept op behind this point reads the value now on this
 * index".  Before the first mark feed it is 1 exactly on the indices of the two output lists.
 *
 * THE WINDOW STEP, for a window [lo, hi) and the needed table N as it stands at hi:
 *   1. every read of the window is resolved to the last writer of its index inside the window and before the reader; a read with no
 *      such writer ESCAPES the window;
 *   2. one count per resolved read on the value it names, and one more on the window's LAST writer of index w when N[w] is set;
 *   3. the peeling of rv_ops_prune_device: the first frontier is every defining op that is no root and has count 0, and so on;
 *   4. unread Inputs are the Input ops whose count stayed 0;
 *   5. KILL, THEN GEN, in that order: N[w] = 0 for every index w that any op of the window writes, kept or dropped; then N[w] = 1
 *      for every escaping read of every kept op (a kept B2A may gen up to 64 indices).  A window that holds "kept op reads w; later
 *      op writes w" leaves N[w] = 1;
 *   6. the window's keep flags go to one mark byte per op, at the ops' ordinals.
 *
 * THE CALLS:  begin -> scan* -> scan_end -> mark* (windows LAST to FIRST, each window's ops in list order) -> mark_end
 *             -> feed* [-> rewind -> feed*]... -> destroy.   The three passes may be cut differently; feeds of 0 and 1 ops are allowed
 * everywhere.  `ops` is host memory (uploaded for the call) or, with ops_on_device, memory of the context's device with
 * rv_ops_prune_device's conventions.
 *   begin     copies the two output lists.
 *   scan      the forward pass: it validates as rv_ops_prune does, the counts in force carried from feed to feed (a backward pass
 *             cannot know the count in force at an op), and refuses a bad list with the code of the first bad op in op order, at
 *             the feed that holds it; it counts the ops and sums the position-keyed digest rv_compactor_* uses.  It writes nothing.
 *   scan_end  fixes the list's length and the final counts; an output index at or above its domain's final count is RV_E_ARG; the
 *             needed tables and the marks are allocated.
 *   mark      a feed covers the ordinals [pos - n_ops, pos), pos starting at the list's length; more ops than are left is RV_E_ARG.
 *             Every index is checked against the final counts before it is used as an address; a record that fails is RV_E_ARG
 *             (not the scanned list) and nothing is addressed by it.  *n_kept_here (may be NULL) receives the feed's kept ops.
 *   mark_end  RV_E_ARG if the pass stopped short of ordinal 0 or its digest is not the scan's.  The info's class counts are
 *             rv_ops_prune's; device_rounds is the SUM of the layers peeled over all mark feeds -- for one feed that holds the whole
 *             list rv_ops_prune_device's figure, otherwise it depends on the cuts; on_device is 0 if any feed fell back (a mark feed
 *             whose peeling reaches RV_PRUNE_MAX_ROUNDS layers is copied down with the two tables, stepped on the host and its marks
 *             and tables uploaded: the bytes are the same, the other feeds stay on the device).
 *   feed      a forward pass: the feed's kept records go to d_out (cap records), their ordinals IN THE WHOLE OLD LIST to d_old_index
 *             (cap entries; may be NULL), the number to *n_out.  cap >= n_ops always suffices; a cap below the kept count is RV_E_ARG
 *             with nothing written.  Any overlap of d_out with a device `ops` is RV_E_ARG before a launch.  The last feed of a pass
 *             answers RV_E_ARG when the pass's digest is not the scan's.
 *   rewind    after a complete emit pass: the next feed is the list's first again.  RV_E_ARG after a short pass.
 * A call out of order is RV_E_ARG and leaves the object as it was.  2^31 ops or more in all, or a final wire count of 2^31 or more:
 * RV_E_UNSUPPORTED.  After a validation code, RV_E_UNSUPPORTED, RV_E_NOMEM or RV_E_DEVICE only destroy is accepted.
 * MEMORY, from the context arena.  Held between calls (state_bytes): one byte per wire index of both domains (final counts), one mark
 * byte per op, and the words.  Per feed, given back before the call returns (peak_feed_bytes: the largest so far): what
 * rv_ops_prune_device takes for a list of the feed's length, plus 24 bytes per op of an uploaded host feed. */
typedef struct rv_pruner rv_pruner;
typedef struct rv_pruner_info {
    uint64_t total_ops;       /* the list's length (before scan_end: the ops scanned so far) */
    uint64_t n_kept;          /* kept ops marked so far (after mark_end: of the list) */
    uint64_t state_bytes;     /* device memory held between calls */
    uint64_t peak_feed_bytes; /* the largest work memory of one call so far, an uploaded feed included */
    uint64_t mark_feeds;      /* mark feeds that held an op */
    uint64_t host_feeds;      /* of these: stepped on the host (the fall-back) */
} rv_pruner_info;             /* 48 bytes */
int rv_pruner_begin(rv_ctx *ctx, size_t z64_wires, size_t gf2_wires, const uint32_t *outputs_gf2, size_t n_outputs_gf2,
                    const uint32_t *outputs_z64, size_t n_outputs_z64, rv_pruner **out);
int rv_pruner_scan(rv_pruner *p, const rv_op *ops, size_t n_ops, int ops_on_device);
int rv_pruner_scan_end(rv_pruner *p);
int rv_pruner_mark(rv_pruner *p, const rv_op *ops, size_t n_ops, int ops_on_device, size_t *n_kept_here);
int rv_pruner_mark_end(rv_pruner *p, rv_prune_info *info /* may be NULL */);
int rv_pruner_feed(rv_pruner *p, const rv_op *ops, size_t n_ops, int ops_on_device, rv_op *d_out, size_t cap, size_t *n_out,
                   uint32_t *d_old_index);
int rv_pruner_rewind(rv_pruner *p);
int rv_pruner_get_info(const rv_pruner *p, rv_pruner_info *info);
void rv_pruner_destroy(rv_pruner *p);
/* host only, no GPU: the three passes over the windows [0, cuts[0]), [cuts[0], cuts[1]), .. [cuts[n_cuts - 1], n_ops) -- the window
 * step's definition in C.  cuts: n_cuts non-decreasing positions, none above n_ops (RV_E_ARG otherwise).  Everything else, and every
 * byte of the result, is rv_ops_prune's (which is this call without a cut). */
int rv_ops_prune_windows_host(const rv_op *ops, size_t n_ops, size_t z64_wires, size_t gf2_wires, const uint32_t *outputs_gf2,
                              size_t n_outputs_gf2, const uint32_t *outputs_z64, size_t n_outputs_z64, const size_t *cuts, size_t n_cuts,
                              rv_op *out, size_t cap, size_t *n_out, uint32_t *old_index, rv_prune_info *info);

/* ---- the same folding for a list that passes through in windows -------------------
 * rv_folder_* gives, for a list that arrives in feeds, exactly rv_ops_fold's records and counts, for every list and every way of
 * cutting it.  Values, reads, the known rule and the rewrite are the ones above.  Folding is a forward data-flow problem, so one
 * pass suffices; what one window tells the next is one KNOWN byte and one 64-bit VALUE per wire index and domain: the state of the
 * last value defined on the index so far.  The tables follow the counts in force and grow when a SizeHint raises one; every entry
 * starts known, value 0 -- the zero wire: a read of an index no earlier op of the LIST wrote is known 0, as in rv_ops_fold.
 *
 * THE WINDOW STEP, for a feed [lo, hi) and the tables K, V as they stand at lo:
 *   1. the feed is validated as rv_ops_fold validates, the counts in force carried from feed to feed; the first bad op in op order
 *      gives its code at the feed that holds it, nothing is written for that feed, and only destroy is accepted afterwards;
 *   2. every read is resolved to the last writer of its index inside the window and before the reader; a read with no such writer
 *      ESCAPES the window, and is known exactly if K[domain][index] is set, with the value V[domain][index];
 *   3. seed, pairs, propagation and rewrite are rv_ops_fold_device's, escaping reads taken from the tables: an op with an unknown
 *      escaping read is never known because its other reads are (a Mul with a known 0 read still is; a B2A needs all 64 either way);
 *   4. AFTER the rewrite has read the tables: for every index any op of the window writes, the window's LAST writer's (known, value)
 *      goes to the tables (value 0 where it is not known).  An index read as escaping and written later in the window ends on the
 *      writer's state;
 *   5. n_known and the nine class counts add up over the feeds.
 * device_rounds is the SUM of the layers over the feeds -- for one feed that holds the whole list rv_ops_fold_device's figure,
 * otherwise it depends on the cuts; on_device is 0 if any feed fell back (a feed whose propagation reaches RV_FOLD_MAX_ROUNDS layers
 * is copied down with the tables, stepped on the host and its records, tables and log entries uploaded: the bytes are the same, the
 * other feeds stay on the device).  The shortcut of a feed is "no op known at once and no escaping read that is known": the records
 * are copied; the tables are updated all the same.
 *
 * THE LOG (RV_FOLDER_KEEP_LOG) answers passes that do not run forwards -- rv_pruner_mark reads its windows from the last to the
 * first.  Every record the rewrite changed is appended to a log in device memory as (ordinal in the whole list, new record),
 * ascending by ordinal.  A replay of ANY window [first, first + n) of the source finds its slice of the log by two lower bounds,
 * copies the source records to d_out unless in place, and stores the slice's records over them.  It propagates nothing and reads
 * no table.
 *
 * THE CALLS:  begin -> feed* -> end [-> rewind -> feed* -> end]... ; after an end, with the log: replay* -> replay_end, any number
 *             of rounds -> destroy.   Feeds of 0 and 1 ops are allowed.  `ops` is host memory (uploaded for the call) or, with
 * ops_on_device, memory of the context's device with rv_ops_fold_device's conventions, checked before any launch.
 *   feed        d_out: device memory for n_ops records; NULL counts (and logs) only; d_out == a device `ops` folds in place; any other
 *               overlap is RV_E_ARG.  In a pass after a rewind, more ops than the first pass had is RV_E_ARG, and the feed that
 *               reaches the list's length answers RV_E_ARG when the pass's position-keyed digest (rv_compactor_*'s) is not the first
 *               pass's.
 *   end         fixes the length and the digest (first pass), fills the info (may be NULL) with this pass's counts.  After a rewind:
 *               RV_E_ARG when the pass stopped short.
 *   rewind      after end: the tables back to known 0, the counts in force back to the declared ones, the log emptied; the next
 *               feed is op 0 again.
 *   replay      needs the log; after end; windows in any order; d_out as for feed, but not NULL.  A window beyond the list is
 *               RV_E_ARG.
 *   replay_end  RV_E_ARG unless the replays since the last replay_end (or end) covered every ordinal exactly once and their digest
 *               is the folded pass's.  The next round begins either way.
 * A call out of order is RV_E_ARG and leaves the object as it was.  2^31 ops or more in all or in one feed, or a wire count in force
 * of 2^31 or more: RV_E_UNSUPPORTED.  After a validation code, RV_E_UNSUPPORTED, RV_E_NOMEM or RV_E_DEVICE only destroy is accepted.
 * MEMORY, from the context arena.  Held between calls (state_bytes): nine bytes per table entry of both domains, and the words; the
 * tables begin at the declared counts, and one that a SizeHint outgrows at least doubles (at most twice nine bytes per wire index).  The
 * log (log_bytes): 28 bytes per entry of its capacity, which doubles when it is full -- at most twice 28 bytes per rewritten op above
 * the first 1024 entries, and nothing per op that is not rewritten.  Per call, given back before it returns (peak_feed_bytes: the
 * largest so far): what rv_ops_fold_device takes for a list of the feed's length, plus 24 bytes per op of an uploaded host feed. */
#define RV_FOLDER_KEEP_LOG 1u
typedef struct rv_folder rv_folder;
typedef struct rv_folder_info {
    uint64_t total_ops;       /* the list's length (before the first end: the ops fed so far) */
    uint64_t state_bytes;     /* device memory held between calls, the log apart */
    uint64_t log_bytes;       /* device memory of the log */
    uint64_t log_records;     /* records in the log: after end, rv_fold_info's n_rewritten */
    uint64_t peak_feed_bytes; /* the largest work memory of one call so far, an uploaded feed included */
    uint64_t feeds;           /* feeds that held an op, over all passes */
    uint64_t host_feeds;      /* of these: stepped on the host (the fall-back) */
} rv_folder_info;             /* 56 bytes */
int rv_folder_begin(rv_ctx *ctx, size_t z64_wires, size_t gf2_wires, uint32_t flags, rv_folder **out);
int rv_folder_feed(rv_folder *f, const rv_op *ops, size_t n_ops, int ops_on_device, rv_op *d_out);
int rv_folder_end(rv_folder *f, rv_fold_info *info /* may be NULL */);
int rv_folder_rewind(rv_folder *f);
int rv_folder_replay(rv_folder *f, const rv_op *ops, size_t n_ops, int ops_on_device, uint64_t first_ordinal, rv_op *d_out);
int rv_folder_replay_end(rv_folder *f);
int rv_folder_get_info(const rv_folder *f, rv_folder_info *info);
void rv_folder_destroy(rv_folder *f);
/* host only, no GPU: the forward sweep over the windows [0, cuts[0]), [cuts[0], cuts[1]), .. [cuts[n_cuts - 1], n_ops) with one
 * state -- the window step's definition in C.  cuts: n_cuts non-decreasing positions, none above n_ops (RV_E_ARG otherwise).
 * Everything else, and every byte of the result, is rv_ops_fold's (which is this call without a cut). */
int rv_ops_fold_windows_host(const rv_op *ops, size_t n_ops, size_t z64_wires, size_t gf2_wires, const size_t *cuts, size_t n_cuts,
                             rv_op *out, rv_fold_info *info);

/* ---- parity-test hooks: each mirrors one reference function so tests can compare the
 * HIP path with the oracle piecewise ---- */
/* PRG::new + gen (crypto/prg.rs:16-37) on the GPU: n_keys keys, blocks [first, first+n_blocks) each */
int rv_hook_prg_blocks(rv_ctx *ctx, const uint8_t *keys, size_t n_keys, uint64_t first_block, size_t n_blocks,
                       uint8_t *out /* n_keys x n_blocks x 16 */);
/* expand_seed (transcript/mod.rs:99-106) for n seeds -> n x 8 x 16 key bytes */
int rv_hook_expand_seed(rv_ctx *ctx, const uint8_t *seeds, size_t n, uint8_t *keys);
/* ShareGen<GF2>::next() x n for one packed group (generator/share.rs:54-65): keys 8x8x16,
 * omit[8] (8 = none) -> n packed u64 shares in the reference's bit order */
int rv_hook_sharegen_gf2(rv_ctx *ctx, const uint8_t *keys, const uint32_t omit[8], size_t n, uint64_t *out);
/* ShareGen<Z64>::next() x n -> n x 8 x 8 u64 */
int rv_hook_sharegen_z64(rv_ctx *ctx, const uint8_t *keys, const uint32_t omit[8], size_t n, uint64_t *out);
/* One mask generator as a shard of R repetitions launches it (R a multiple of 8, at most 256; rows of R/4 quad words), on CTR blocks
 * [first_block, first_block + n_blocks) of the 8 R player keys of seeds [R][16].
 *   omit       [R], 0..7 = the player whose stream stays zero, 8 = none; NULL = the prover's launch (no keep words at all)
 *   generator  0 = the 128-plane GF(2) generator, 1 = the lane-distributed GF(2) generator, 2 = the Z64 generator
 *   key_path   0 = expand_seeds + key_schedule + bitslice_rk (+ the lane-distributed key image), 1 = the one-launch key setup
 *   out        the device rows as they are: GF(2) uint32 [n_blocks * 128][R/4], Z64 uint64 [2 * n_blocks][8 R]
 * Checked before anything is launched: RV_E_UNSUPPORTED for generator 1 at a width it does not take (R/4 not a multiple of 16) and for
 * first_block + n_blocks > 2^24; RV_E_ARG for any other R, an omit value above 8, n_blocks == 0, an unknown generator or key path. */
int rv_hook_maskgen(rv_ctx *ctx, const uint8_t *seeds, uint32_t R, const uint8_t *omit, uint32_t generator, uint32_t key_path,
                    uint64_t first_block, uint64_t n_blocks, void *out);
/* ---- the opening and unpacking kernels, one production launch each on caller-supplied data (csrc/open.hip, csrc/z64.hip; the Pack /
 * PackSelected implementations of algebra/gf2/{share,recon}.rs and algebra/z64/{share,recon}.rs).  A shard of R repetitions (a multiple
 * of 8, at most 256) has rows of NQ = R/4 quad words; omit[R] holds 0..7 = the opened repetition's omitted player, 8 = not opened.
 * Every output buffer is read first and returned whole, so a byte the launch does not write keeps the caller's fill.  All of them
 * return RV_E_ARG before anything is launched for an R that is not as above, an omit value above 8, more than RV_ONLINE_REPS opened
 * repetitions (the kernels clamp there and no caller exceeds it), or a vector that does not lie inside its buffer. ---- */
/* launch_extract_bits: the opened repetitions' packed vectors (n_items / 8 + 1 bytes, item i at bit 7 - i % 8 of byte i / 8) of items
 * rows[0 .. n_items) (NULL: 0, 1, ...) of stream [stream_rows][NQ] u32, repetition r's at out + dst_off[r].  kind 0: the omitted player's
 * bit of a share row; 1: a reconstruction row's 0x00 / 0xFF byte.  out2 (kind 0; NULL or out_bytes like out) and n_direct: the first
 * n_direct tiles also go, in whole aligned 16-byte words, to out2.  gaps (NULL or 8 words; needs out2): k_copy_gaps then copies the
 * image `out` into out2 around the corrections vectors of the first opened records -- gaps = {first, rec, corr_at, corr_len, n_rec,
 * rep_limit, rvec_at, od}: n_rec <= 40 records of rec bytes from byte `first`, the corrections at [corr_at, corr_at + corr_len) of each,
 * left out for the opened repetitions below rep_limit <= 256; od != 0: it also leaves out the words the extraction has sent, the
 * vectors lying at rvec_at of their records (dst_off[r] = first + j * rec + rvec_at for the j-th opened repetition is the caller's
 * part).  *tile = the tile of the launch in bytes. */
int rv_hook_extract_bits(rv_ctx *ctx, const uint32_t *stream, uint64_t stream_rows, const uint32_t *rows, uint64_t n_items, uint32_t R, int kind,
                         const uint8_t *omit, const uint64_t *dst_off, uint8_t *out, uint64_t out_bytes, uint8_t *out2, uint32_t n_direct,
                         const uint64_t *gaps, uint32_t *tile);
/* launch_extract_from_bits: the same vectors from a bit-per-repetition stream [n_items][R/8] bytes (bit k of nibble q of a row =
 * repetition 4q + 3 - k), through the list of opened repetitions as the challenge kernel builds it from omit and dst_off; the
 * repetitions below rep_min are left out.  *tile as above. */
int rv_hook_extract_from_bits(rv_ctx *ctx, const uint8_t *bits, uint64_t n_items, uint32_t R, const uint8_t *omit, const uint64_t *dst_off,
                              uint32_t rep_min, uint8_t *out, uint64_t out_bytes, uint32_t *tile);
/* launch_pack_corr_all: bytes [byte0, byte0 + n_bytes) of ALL 256 repetitions' vectors of a stream [n_items][32], repetition r's at
 * out + r * pitch; out is 256 * pitch bytes.  The kernel writes whole 16-byte words: up to 15 bytes behind n_bytes are padding.
 * RV_E_ARG for a pitch that is not a multiple of 128 (or above 2^24) and for n_bytes > pitch. */
int rv_hook_pack_corr_all(rv_ctx *ctx, const uint8_t *bits, uint64_t n_items, uint64_t byte0, uint64_t n_bytes, uint64_t pitch, uint8_t *out);
/* launch_unpack_bits: rows_out [n_items][out_nq] u32 from the opened repetitions' vectors at blob + src_off[r], src_len[r] bytes each
 * (items past a vector's end are zero); row 0 is item first_item of the vectors.  out_nq = R/4, or 16 when R > 64 and no repetition
 * from 64 on is opened (RV_E_ARG otherwise: the kernel relies on it). */
int rv_hook_unpack_bits(rv_ctx *ctx, const uint8_t *blob, uint64_t blob_bytes, const uint64_t *src_off, const uint64_t *src_len, const uint8_t *omit,
                        uint64_t n_items, uint32_t R, int kind, uint32_t out_nq, uint64_t first_item, uint32_t *rows_out);
/* launch_extract64: 8 bytes little-endian per item, word offs[i] (NULL: i) + (add_omit ? omit[r] : 0) of repetition r's stream
 * [R][stride_words] u64, to out + dst_off[r].  use_list = 0: the kernel with a thread per (repetition, item); 1: the one over the list
 * of opened repetitions, which leaves out those below rep_min. */
int rv_hook_extract64(rv_ctx *ctx, const uint64_t *stream, uint64_t stride_words, const uint64_t *offs, uint64_t n_items, int add_omit, uint32_t R,
                      const uint8_t *omit, const uint64_t *dst_off, int use_list, uint32_t rep_min, uint8_t *out, uint64_t out_bytes);
/* launch_unpack64: out [n_items][out_r] u64 from vectors of 8-byte items as above (an item that is not whole reads as zero).
 * out_r = R, or 64 when R > 64 and no repetition from 64 on is opened (RV_E_ARG otherwise). */
int rv_hook_unpack64(rv_ctx *ctx, const uint8_t *blob, uint64_t blob_bytes, const uint64_t *src_off, const uint64_t *src_len, const uint8_t *omit,
                     uint64_t n_items, uint32_t R, uint32_t out_r, uint64_t *out);
/* The gate-stream compiler alone (host only, no device: ctx-free): what rv_circuit_compile_ex would report through
 * rv_circuit_get_info -- the counters that are pure functions of the op list (ShareGen::next() calls per repetition,
 * generator/share.rs:54-65; transcript events, prover.rs:194,210,216), dependency levels, operand rows -- and the errors the
 * reference raises while stepping (wire out of range, bad op).  device_bytes / scratch_bytes / upload_us stay zero.
 * chunk_first_ops (0 = off): also checks, like a streaming feed cut every that many ops would, that every piece compiled
 * on its own with the ShareGen phases predicted from the ops before it adds up to the whole (RV_E_DEVICE if not). */
int rv_hook_compile_info(const rv_op *ops, size_t n_ops, size_t z64_wires, size_t gf2_wires, uint32_t flags, size_t chunk_ops,
                         rv_circuit_info *info);
/* The level table of the gate stream and the plan that assigns its levels to executors (host only, no device; the compile of
 * rv_hook_compile_info).  out: ten int32 per level, the first `cap` levels -- the class bounds lo, mul11, mul, xor2, xork, hi of the
 * level's gates (csrc/internal.h: LevelRange; one-base Mul, other Mul, two-base XorK, other XorK, everything else), 1 when the level
 * holds Z64 gates, the index of the narrow run the level belongs to and that run's kind (1 per-gate, 0 class-loop, 2 lean; -1 and -1
 * when the level is launched on its own), -1.  *n_levels: the levels there are.  The plan is computed by the function the upload
 * path calls. */
int rv_hook_compile_levels(const rv_op *ops, size_t n_ops, size_t z64_wires, size_t gf2_wires, uint32_t flags, int32_t *out, size_t cap,
                           size_t *n_levels);
/* The same table of a compiled circuit; its tenth column is the index of the LDS run that holds the level (-1: none), planned for the
 * LDS size of the circuit's context.  *vclr_ok (nullable): the circuit qualifies for MODE_PROVE_V; *general_levels (nullable): some
 * level takes the kernel variant with the multi-base loops, which rules MODE_VERIFY_C out. */
int rv_hook_circuit_levels(const rv_circuit *c, int32_t *out, size_t cap, size_t *n_levels, int *vclr_ok, int *general_levels);
/* Launches of the GF(2) level executors this process has issued so far (relaxed atomic counters, bumped by the host launchers), eleven
 * rows of four: rows = own launch fast, own launch general, generic k_interp, narrow per-gate, narrow class-loop, narrow lean, LDS run,
 * batched full, batched narrow per-gate, batched narrow class-loop, batched LDS; columns = the kernel's mode PROVE, PROVE_V, VERIFY,
 * VERIFY_C.  reset != 0: the counters return to zero as they are read. */
int rv_hook_interp_launches(uint64_t counts[][4], int reset);
/* Launches of the Z64 level executors this process has issued so far, counted by the host launchers (one that returns early -- an
 * empty level, no quad group -- counts nothing), four rows of two: rows = k_z64_fused in blocks of 16 quad words, k_z64_fused in
 * blocks of 8, k_interp64, k_interp64_b (batches); columns = prover, verifier.  reset != 0: the counters return to zero as they are
 * read. */
int rv_hook_interp64_launches(uint64_t counts[][2], int reset);
/* The grid of one k_z64_fused launch (host only; the function the launcher calls): for a level of n_mul Mul, n_lin linear and
 * n_oth other gates over n_qg quad groups of qw (16 or 8) quad words on `cus` compute units (0: what the launcher uses on this
 * machine, 256 where no device answers) -- out = chunks (workgroups per quad group; 0: nothing is launched), mul_per, lin_per,
 * oth_per (a workgroup's share of each class), lin_bias. */
int rv_hook_z64_fused_grid(uint32_t qw, uint32_t n_qg, uint32_t cus, uint32_t n_mul, uint32_t n_lin, uint32_t n_oth, uint32_t out[5]);
/* The fused Z64 level table of a program (host only; the compile of rv_hook_compile_levels, then the function the upload path
 * calls).  out: four uint32 per level, the first `cap` levels -- mul0, mul1, lin1, oth1: Mul gates [mul0, mul1), Add .. MulConst
 * [mul1, lin1), Input / AssertZero / Const [lin1, oth1).  *eligible: 0 the circuit takes the fused path; 1 it holds a Random or
 * B2A gate (no table: *n_levels = 0); 2 a Mul's mask pair straddles cipher blocks; 3 more than 64 Input block runs; 4 no Z64 gate. */
int rv_hook_z64_fused_levels(const rv_op *ops, size_t n_ops, size_t z64_wires, size_t gf2_wires, uint32_t flags, uint32_t *out, size_t cap,
                             size_t *n_levels, int *eligible);
/* What the upload path makes of a program for the fused Z64 path (host only; the same compile, then the same function): the records
 * grouped Mul | linear | other inside every level (64 bytes each, the layout of csrc/internal.h: Gate64), the level table as above, the
 * cipher block runs whose rows are Input masks (two uint64 per run: first block, blocks) and the eligibility code as above.  Count,
 * then fill: *n_gates, *n_levels and *n_runs are always the full counts, every array takes its first `cap` entries.  sizes (nullable):
 * Z64 SSA ids, mask rows, online and preprocessing words per repetition, input, correction and reconstruction ordinals. */
int rv_hook_z64_fused_gates(const rv_op *ops, size_t n_ops, size_t z64_wires, size_t gf2_wires, uint32_t flags, void *gates, size_t gates_cap,
                            size_t *n_gates, uint32_t *levels, size_t levels_cap, size_t *n_levels, uint64_t *runs, size_t runs_cap,
                            size_t *n_runs, int *eligible, uint64_t sizes[7]);
/* One fused Z64 level launch after the other on caller-supplied records and buffers (tests/test_gpu_z64_fused_level.py, reference
 * tests/z64f_ref.py): the production launcher, once per level of `levels` in order, over quad groups [qg0, qg0 + qgn) of the rows'
 * R / 4 quad words, the cipher counting from first_block.  omit = NULL: the prover (wit, v); else the verifier (omit[R] = 0..7 the
 * hidden player of an opened repetition, 8 not opened; wcorr and the three supplied arrays [ordinal][sup_r]).  Keys come from
 * seeds[R][16] by the three set-up launches (key_path 0) or the fused one (1); the rows of the block runs are generated from
 * first_block + first with the verifier's keep words, as a shard does, before the first level.  wmask [n_ssa][8 R], masks
 * [n_mask_rows][8 R], v [n_ssa], wcorr [n_ssa][R], on [R][on_words], pre [R][pre_words] and err [1] are read first and come back
 * whole.  RV_E_ARG, with nothing written: R / 4 is no multiple of 8, the quad groups leave the row, a level leaves the records, a
 * record of the wrong class or a Random / B2A record, a Mul with odd m, any index of a record that leaves its buffer, an opened
 * repetition at or past sup_r.  RV_E_UNSUPPORTED, with nothing written: a counter first_block + m / 2 of 2^24 or more. */
typedef struct rv_hook_z64f_run_args {
    const uint8_t *seeds;
    const uint8_t *omit;
    uint32_t R, key_path;
    uint64_t first_block;
    uint32_t qg0, qgn;
    const void *gates;
    size_t n_gates;
    const uint32_t *levels; /* [n_levels][4] */
    size_t n_levels;
    const uint64_t *runs; /* [n_runs][2] */
    size_t n_runs;
    uint64_t on_words, pre_words;
    const uint64_t *wit;
    size_t n_wit;
    const uint64_t *sup_in, *sup_corr, *sup_rec;
    size_t n_in, n_corr, n_rec;
    uint32_t sup_r, reserved;
    size_t n_ssa, n_mask_rows;
    uint64_t *wmask, *masks, *v, *wcorr, *on, *pre;
    int32_t *err;
} rv_hook_z64f_run_args;
int rv_hook_z64_fused_run(rv_ctx *ctx, const rv_hook_z64f_run_args *args);
/* The transcript-hash kernels (BLAKE3 chunk kernels, trees, the incremental tree, the digest join), one production launch at a time
 * on caller-supplied data (tests/test_gpu_b3_kernels.py, reference tests/b3_ref.py).  Kernel numbers -- chunk kernels: 1 a repetition
 * per lane, 2 a quad word per lane, 3 a chunk per wavefront (rows of 64 quad words, no quad list); tree tops: 1 a lane per repetition,
 * 2 the 64-node workgroup top, 3 the 512-node one; small pair: 1 a quad of lanes per compression, 2 a lane per repetition.
 * `choice` = 0: production's own pick; else that kernel through the launch code production runs after picking -- RV_E_ARG, before
 * anything is launched, when the kernel does not take the shape.  `batch` = 0: launched directly; 2..64: recorded that many times on
 * as many inputs laid end to end, then replayed as one batch (the launchers see the batch).  Every output buffer is filled with 0xA5
 * before the launch and returned whole, its size per input given by the caller (at least what the launch writes).
 * rv_hook_b3_plan (host only): what production picks for a preprocessing stream of n_pre and an online stream of n_on events in rows
 * of NQ quad words (`listed`: the online stream with a quad list of n_quads words), with a recorder of that batch (0: none) --
 * out = online chunk kernel (0: nothing launched), preprocessing chunk kernel, {reduction launches, nodes at the top, top kernel} of
 * the online and of the preprocessing tree, small pair (0: not taken), big pair taken, its launches, its two streams' nodes at the
 * shared top (preprocessing, online). */
int rv_hook_b3_plan(uint64_t n_pre, uint64_t n_on, uint32_t NQ, int listed, uint32_t n_quads, uint32_t batch, uint32_t out[13]);
/* kind 0: byte rows [n][width] u32; 1: bit rows [n][width / 2] u8 (width = NQ); 2: contiguous streams [width][stride_words] u64 of which
 * n words are hashed (width = R; choice must be 0) -> cvs [n_chunks][R][8] in front of cv_words words; *chosen: the kernel launched. */
int rv_hook_b3_chunks(rv_ctx *ctx, int kind, const void *stream, uint64_t n, uint32_t width, uint64_t stride_words, const uint32_t *quads,
                      uint32_t n_quads, uint64_t chunk_base, uint32_t root_ok, uint32_t choice, uint32_t batch, uint32_t *cvs, uint64_t cv_words,
                      uint32_t *chosen);
/* Both transcripts of a small proof in two shared launches: chaining values and digests of both; *taken = 0: the launcher declined. */
int rv_hook_b3_pair_small(rv_ctx *ctx, const uint8_t *pre, uint64_t n_pre, const uint32_t *on, uint64_t n_on, uint32_t NQ, const uint32_t *quads,
                          uint32_t n_quads, uint32_t choice, uint32_t batch, uint32_t *cv_pre, uint64_t cv_pre_words, uint32_t *cv_on,
                          uint64_t cv_on_words, uint32_t *dig_pre, uint32_t *dig_on, uint64_t dig_words, uint32_t *taken);
/* The shared chunk launch of a large proof's two transcripts (rows of 64 quad words). */
int rv_hook_b3_pair_big_chunks(rv_ctx *ctx, const uint8_t *pre, uint64_t n_pre, const uint32_t *on, uint64_t n_on, const uint32_t *quads, uint32_t n_quads,
                               uint32_t *cv_pre, uint64_t cv_pre_words, uint32_t *cv_on, uint64_t cv_on_words);
/* The tree over cvs [n][R][8]; plan[3] = reduction launches, nodes at the top, top kernel. */
int rv_hook_b3_tree(rv_ctx *ctx, const uint32_t *cvs, uint64_t n, uint32_t R, uint32_t choice, uint32_t batch, uint32_t *digest, uint64_t dig_words,
                    uint32_t plan[3]);
/* The two trees of a large proof in shared launches. */
int rv_hook_b3_pair_big_tree(rv_ctx *ctx, const uint32_t *cvs_a, uint64_t n_a, const uint32_t *cvs_b, uint64_t n_b, uint32_t R, uint32_t *dig_a,
                             uint32_t *dig_b, uint64_t dig_words, uint32_t *launches);
/* The streaming prover's incremental tree over B streams (cvs [B][n][R][8]): n - 1 values absorbed in pieces, the last one closes. */
int rv_hook_b3_incremental(rv_ctx *ctx, const uint32_t *cvs, uint64_t n, uint32_t R, uint32_t B, const uint64_t *pieces, uint32_t n_pieces,
                           uint32_t *digest, uint64_t dig_words);
/* The digest join: digs [4][R][8] (pre2, on2, pre64, on64) -> h [R][32] in front of h_bytes bytes. */
int rv_hook_b3_join(rv_ctx *ctx, const uint32_t *digs, uint32_t R, uint32_t batch, uint8_t *h, uint64_t h_bytes);
/* ---- Fiat-Shamir, the record heads, the framing and the set-up kernels (csrc/open.hip), one production launch each on caller-supplied
 * data (csrc/hooks_open.inc; proof/mod.rs:41-108, crypto/ro.rs:8-20).  As above: every output buffer is read first and returned whole,
 * and RV_E_ARG is returned before anything is launched for whatever a kernel relies on its callers for. ---- */
/* launch_fs_challenge on digests [B][256][32] (B = batch, or 1 when batch is 0) for the shard (rep_begin, R): both multiples of 8 inside
 * the 256 repetitions.  layout[10] = the section starts base[4], then sz2, sz64, l2r, l2c, l64r, l64c (record sizes and vector byte
 * lengths); framed (0 / 1; 1 only for the whole shard): base[1..3] are taken as given instead of following from the device's counts.
 * flags: bit 0 omit_all, bit 1 res, bit 2 comm2, bit 3 the mailbox are passed to the kernel (NULL otherwise; the mailbox not in a batch).
 * Outputs, B of each: comm [32], omit [R], omit_all [256], offs [8][R], ol (the kernel's list of opened repetitions, 488 bytes: u32 n,
 * u32 rep[40], four bytes of padding, u64 dst[40]), res [2], comm2 [32]; mbox [128] words of host-mapped memory: word 0 receives
 * mbox_seq, words 16 .. 89 comm, the whole map and the two counts.  batch >= 2: recorded and replayed as a batch of proofs is. */
int rv_hook_fs_challenge(rv_ctx *ctx, const uint8_t *digests, const uint64_t *layout, uint32_t framed, uint32_t rep_begin, uint32_t R, uint32_t flags,
                         uint32_t mbox_seq, uint32_t batch, uint8_t *comm, uint8_t *omit, uint8_t *omit_all, uint64_t *offs, uint8_t *ol, uint32_t *res,
                         uint8_t *comm2, uint32_t *mbox);
/* launch_open_headers: the fixed-size parts of a shard's records into out -- seeds [R][16], keys [R][128], on2 / on64 [R][8] u32 (the
 * online transcripts' digests), off2 / off64 [R] the records' offsets, lens[6] = l2r, l2c, l2i, l64r, l64c, l64i.  RV_E_ARG for a record
 * that does not lie inside out. */
int rv_hook_open_headers(rv_ctx *ctx, uint32_t R, const uint8_t *omit, const uint8_t *seeds, const uint8_t *keys, const uint32_t *on2, const uint32_t *on64,
                         const uint64_t *off2, const uint64_t *off64, const uint64_t *lens, uint8_t *out, uint64_t out_bytes);
/* launch_open_small: the heads as above from the table offs [8][R], and the three GF(2) vectors: rows rec_rows[0 .. n_rec) and
 * in_rows[0 .. n_in) (NULL: 0, 1, ...) of stream [stream_rows][R/4] u32, n_pre rows of the bit stream pre [n_pre][R/8] through the list ol
 * (488 bytes as rv_hook_fs_challenge returns them), without the repetitions below corr_rep_min.  flags: bit 0 heads_inputs_only, bit 1
 * the host-mapped error word is passed and receives err_src.  *taken = 0: the launcher declined and nothing ran; tiles[3]: the tiles of
 * the three extractions in bytes. */
int rv_hook_open_small(rv_ctx *ctx, uint32_t R, const uint8_t *omit, const uint8_t *seeds, const uint8_t *keys, const uint32_t *on2, const uint32_t *on64,
                       const uint64_t *offs, const uint64_t *lens, const uint32_t *stream, uint64_t stream_rows, const uint32_t *rec_rows, uint64_t n_rec,
                       const uint8_t *pre, uint64_t n_pre, const uint32_t *in_rows, uint64_t n_in, const uint8_t *ol, uint32_t corr_rep_min, int err_src,
                       uint32_t flags, uint8_t *out, uint64_t out_bytes, int *taken, uint32_t *tiles, int *err_word);
/* launch_frame_counts: the four repetition counts of `batch` framed proofs `stride` bytes apart in out; lens[4] the section lengths.
 * *taken = 0: the launcher declined (no proof, an offset or stride that is no multiple of 8) and nothing ran. */
int rv_hook_frame_counts(rv_ctx *ctx, uint8_t *out, uint64_t out_bytes, uint64_t stride, uint32_t batch, const uint64_t *lens, int *taken);
/* launch_overlay_rows: rows of src replace those of dst ([R][row_words] u32) where (omit[r] < 8) == want_online. */
int rv_hook_overlay_rows(rv_ctx *ctx, uint32_t *dst, const uint32_t *src, const uint8_t *omit, uint32_t R, uint32_t row_words, int want_online);
/* launch_fill_digests: n_rows copies of digest[8] at the start of dst (dst_words words). */
int rv_hook_fill_digests(rv_ctx *ctx, uint32_t *dst, uint64_t dst_words, uint32_t n_rows, const uint32_t *digest);
/* launch_shard_init: err[0] (of two ints) cleared, the first n_mask_words of mask and n_corr_bytes of corr cleared (RV_E_ARG above 64: the
 * kernel has 64 threads and no loop), n_fill_rows copies of digest[8] into fill (NULL: none), zero_byte[0] (NULL or 8 bytes) cleared. */
int rv_hook_shard_init(rv_ctx *ctx, int *err, uint32_t *mask, uint64_t mask_words, uint32_t n_mask_words, uint8_t *corr, uint64_t corr_bytes,
                       uint32_t n_corr_bytes, uint32_t *fill, uint64_t fill_words, uint32_t n_fill_rows, const uint32_t *digest, uint8_t *zero_byte);
/* launch_store_words: src [n_words] into dst (dst_words < 1023 words, host-mapped for the launch); with_err: a device word holding
 * err_value into *dst_err. */
int rv_hook_store_words(rv_ctx *ctx, const uint32_t *src, uint32_t n_words, uint32_t *dst, uint32_t dst_words, int err_value, int with_err, int *dst_err);
/* The two gate-stream compilers against each other (host only): the program is compiled by the sequential compiler and by the
 * parallel one with `threads` host threads (>= 2), whatever its size, and the results are compared field by field.
 * *diff = 0: identical; > 0: a number naming the first differing table (csrc/compile_par.cpp, compiled_diff); -1: the parallel
 * compiler declined the program (B2A gates, an error in the op list) -- the sequential result is what rv_circuit_compile uses.
 * Returns the sequential compiler's status (RV_OK or the error the reference raises while stepping, single.rs:106-156). */
int rv_hook_compile_compare(const rv_op *ops, size_t n_ops, size_t z64_wires, size_t gf2_wires, uint32_t flags, int threads, int *diff);
/* The device compiler against the host compiler (compile_ops) on the same program: *path = 1 when the device path compiled it, 0
 * when it handed it to the host compiler; *diff = 0 when the two results are identical field by field (as rv_hook_compile_compare).
 * The hook tries the device whether or not RV_COMPILE_DEVICE is set, except that RV_COMPILE_WHOLE_PROVER without the device bit stays
 * a host compile (*path = 0): with RV_COMPILE_WHOLE_PROVER | RV_COMPILE_DEVICE it tries the device compiler on the lazy-sum form and
 * compares with the host compiler's forced lazy-sum compile.  RV_COMPILE_DEVICE_Z64 (with RV_COMPILE_DEVICE, else RV_E_ARG) lets the
 * device side take Z64 and mixed programs, RV_COMPILE_DEVICE_B2A (with both, else RV_E_ARG) programs with B2A ops,
 * RV_COMPILE_DEVICE_KEEP_WIRES (with RV_COMPILE_KEEP_WIRES and RV_COMPILE_DEVICE, else RV_E_ARG) RV_COMPILE_KEEP_WIRES compiles, whose
 * wire tables are compared too; every other flag value behaves as before.  Returns the host compiler's status. */
int rv_hook_compile_compare_device(rv_ctx *ctx, const rv_op *ops, size_t n_ops, size_t z64_wires, size_t gf2_wires, uint32_t flags, int *path,
                                   int *diff);
/* The same for one piece of a stream: both sides compile the ops as the streaming chunk that starts at `start` = { mask_phase (< 128),
 * mask64_phase (< 2), on0, pre0, on_words64_0, pre_words64_0 } (the ShareGen phases and the carried transcript events in front of the
 * piece's own).  *path, *diff and the return value as rv_hook_compile_compare_device. */
int rv_hook_compile_compare_device_chunk(rv_ctx *ctx, const rv_op *ops, size_t n_ops, size_t z64_wires, size_t gf2_wires, const uint64_t start[6], int *path, int *diff);
/* The same with the stream's compile flags: 0 and RV_COMPILE_DEVICE are the hook above (GF(2) pieces only); RV_COMPILE_DEVICE |
 * RV_COMPILE_DEVICE_Z64 lets the device side take Z64 and mixed pieces, RV_COMPILE_DEVICE_B2A beside both pieces with B2A ops.
 * RV_E_ARG for any other value. */
int rv_hook_compile_compare_device_chunk_ex(rv_ctx *ctx, const rv_op *ops, size_t n_ops, size_t z64_wires, size_t gf2_wires, const uint64_t start[6],
                                            uint32_t flags, int *path, int *diff);
/* Pieces of this process's streams (rv_stream_*, rv_eval_stream_* and the one-shot calls over them) that the device path compiled so
 * far: a test tells a device compile from a fallback to the host compiler by it. */
uint64_t rv_hook_stream_device_chunks(void);
/* out[0] / out[1]: op bytes this process's stream feeds copied host -> device (the pieces a host feed uploads under RV_COMPILE_DEVICE)
 * and device -> host (the pieces of a device feed that the host compiler had to read) since the library was loaded */
int rv_hook_stream_op_traffic(uint64_t out[2]);
/* The eight sums a feed takes from the content of a piece -- digest, GF(2) masks, Z64 masks, in2, rec2, pre2, on64, pre64 -- for
 * every piece of ops [0, n_ops) at stream position first_index, cut every piece_ops ops (0: one piece, also an empty one):
 * host_out from the host feed's loops, dev_out from one launch of the device feed's kernel over all pieces (the ops are uploaded
 * for it); both [pieces][8], pieces = max(1, ceil(n_ops / piece_ops)).  They must agree on every op array, malformed ops included. */
int rv_hook_stream_piece_sums(rv_ctx *ctx, const rv_op *ops, size_t n_ops, uint64_t first_index, size_t piece_ops, uint64_t *host_out,
                              uint64_t *dev_out);
/* Per-phase times of this process's last device compile, ms from HIP events: out[0] classify and count, [1] last writers and consumer
 * lists, [2] values and levels (topological rounds), [3] rows, sort and tables, [4] the host's copy; out[5] = rounds launched. */
int rv_hook_compile_device_laps(double out[6]);
/* RV_COMPILE_DEVICE_Z64, a list with Z64 ops: ms of the split of the list and of the Z64 ops' steps in that compile (0 otherwise);
 * the six figures above are then the GF(2) ops' (RV_COMPILE_DEVICE_B2A: the expansion of the B2A ops is part of the split, their
 * 442 steps each are among the GF(2) ops). */
int rv_hook_compile_device_laps_z64(double *out);
/* DomainGF2::reconstruct (gf2/domain.rs:47-63) on n packed u64 shares (bit 63 - (8*rep + player)) -> n ReconGF2 words
 * (one 0x00/0xFF byte per repetition), through the interpreter's own device function */
int rv_hook_gf2_reconstruct(rv_ctx *ctx, const uint64_t *shares, size_t n, uint64_t *out);
/* DomainZ64::reconstruct (z64/domain.rs:53-61) on n ShareZ64 values ([8 reps][8 players] u64) -> n x 8 wrapping sums */
int rv_hook_z64_reconstruct(rv_ctx *ctx, const uint64_t *shares /* n x 64 */, size_t n, uint64_t *out /* n x 8 */);
/* BLAKE3 of n_streams independent byte strings of equal length len (row-major), on the GPU
 * tree-hash kernels used for the transcripts (crypto/hash.rs:17-57) */
int rv_hook_blake3(rv_ctx *ctx, const uint8_t *data, size_t n_streams, size_t len, uint8_t *out /* n x 32 */);
/* per-stream digests of a committed shard: rep_count x 4 x 32 = H_pre(gf2), H_on(gf2), H_pre(z64), H_on(z64) */
int rv_hook_shard_stream_digests(rv_shard *s, uint8_t *out);
/* Proofs this process has produced through rv_prove's early-corrections path (csrc/api.hip, rv_prove_impl: for large GF(2)
 * circuits the corrections vectors of all repetitions -- Pack of ReconGF2, gf2/recon.rs:189-239, half of what
 * ProverTranscript::extract returns, prover.rs:57-175 -- cross PCIe before the challenge exists).  The bytes are the same
 * either way; the tests use the counter to know which path they compared.  RV_EARLY=0 turns the path off. */
uint64_t rv_hook_early_proofs(void);
/* ... and those of them whose opened repetitions' broadcast vectors (the omitted player's shares, prover.rs:57-175) were written into
 * the page-locked proof buffer by the extraction kernel itself (csrc/internal.h: OpenDirect; RV_OPEN_DIRECT=0/1 turns it off).  Same
 * bytes either way. */
uint64_t rv_hook_open_direct_proofs(void);
/* rv_prove_ops / rv_verify_ops calls of this process that found their op list's compiled circuit in the context's cache (ABI 7). */
uint64_t rv_hook_ops_cache_hits(void);
/* Host only, no device: the comparison a cache lookup of rv_prove_ops / rv_verify_ops decides on -- 1 iff the two ranges hold the same
 * bytes (parallel memcmp, first difference ends it), 0 if not, -1 on a NULL range. */
int rv_hook_ops_same(const void *a, const void *b, size_t bytes);
/* Shard commitments of this process whose GF(2) mask generator ran BESIDE the interpreter's level launches (round 5: the
 * lane-distributed cipher of csrc/aes_col4.hip on a stream of its own, chunk by chunk; RV_OVERLAP=0 runs it before the first level;
 * circuits below RV_OVERLAP_MIN = 8192 cipher blocks and rows narrower than 64 repetitions keep that order anyway).  Same bytes. */
uint64_t rv_hook_overlap_commits(void);
/* Verifications this process has run with one u64 of public corrections per share row instead of corr rows (csrc/interp.hip:
 * MODE_VERIFY_C -- the verify-mode interpreter of whole proofs of pure GF(2) one-base gate streams; replaces nothing of the
 * reference's: verifier/online.rs:122-183 computes the same values).  The answer is the same either way; the tests use the
 * counter to know which path they compared.  RV_VERIFY_VC=0 turns the path off. */
uint64_t rv_hook_verify_vc_count(void);
/* Running total of the proof bytes this process's shard verifiers (rv_verify_shard*, rv_verify_shard_groups, hence rv_verify,
 * rv_verify_sharded) copied host-to-device: the records of the online groups they verified, both domains. */
uint64_t rv_hook_verify_proof_bytes(void);
/* rv_verify_device / rv_verify_sections_device calls of this process that took out[0] = the device path, out[1] = the host fallback
 * (calls refused with RV_E_ARG count as neither). */
int rv_hook_verify_device_paths(uint64_t out[2]);
/* What the single-proof verifiers of this process (rv_verify*, rv_verify_shard*, rv_verify_device, rv_verify_sections_device on
 * the device path) decided about their order of work, as running totals: out[0] = calls, out[1] = every host array and the proof
 * in one copy through the staging buffer, out[2] = the proof's copy on the second stream, out[3] = the fused Z64 verifier's quad
 * groups split around that copy, out[4] = the fused Z64 verifier, out[5] = the GF(2) mask generator beside the levels,
 * out[6] = MODE_VERIFY_C (as rv_hook_verify_vc_count), out[7] = calls whose proof lay in device memory.  The answer is the same on
 * every path; the tests use the counters to know which one a shape took. */
int rv_hook_verify_schedule(uint64_t out[8]);
/* What the provers of this process that commit and open one proof at a time (rv_prove*, rv_prove_device*, rv_prove_ops, a batch
 * proved proof after proof, rv_shard_commit and rv_prove_sharded for their shard) decided, as running totals: out[0] = commitments
 * queued, out[1] = early corrections, out[2] = ... in their Z64 form, out[3] = broadcast vectors written straight into the proof
 * buffer, out[4] = the proof through the mapped staging buffer, out[5] = seeds and GF(2) witness in one page-locked copy,
 * out[6] = MODE_PROVE_V, out[7] = the fused Z64 prover, out[8] = the GF(2) mask generator beside the levels, out[9] = the
 * lane-distributed mask generator; then the form of every openings call (rv_shard_open* included): out[10] = one launch,
 * out[11] = heads and inputs in one launch, out[12] = separate launches, out[13] = the error word sent by that one launch.
 * out[14], out[15] = 0.  The proof is the same on every path; the tests use the counters to know which one a shape took. */
int rv_hook_prove_schedule(uint64_t out[16]);
/* Proofs rv_verify_batch_device verified in this process through out[0] = the one-pass device path, out[1] = the single-proof
 * device verifier, out[2] = a host copy (walks that stopped); calls refused with RV_E_ARG count nowhere. */
int rv_hook_verify_batch_device_paths(uint64_t out[3]);
/* The framing walk of those two entry points, run on the host (no device): bytes[0, len) in framing 0 = bincode(Proof) or 1 = the
 * four sections, whose lengths the caller leaves in table[0 .. 3] (RV_E_ARG unless their sum is len).  table: 657 words (csrc/verify_dev.h)
 * -- record k = 40 * domain + i at words 8k .. 8k + 7: the offsets of keys, rec (then its length), corr (length), in (length), the
 * omit byte; words 640 / 641: where the domains' preprocessing records start; 642: the status; 643 .. 652: the 80 omit bytes;
 * 653 .. 656: comm.  *status: 0 = walked, 1 = the bytes run out, 2 = a count is not 40 / 216, 3 = a section does not end where its
 * records do (or a preprocessing section is not 216 x 48 bytes), 4 = a group's records are refused; words behind a stop are zero. */
int rv_hook_verify_walk(const uint8_t *bytes, size_t len, int framing, uint64_t *table, int *status);
/* How often this process's evaluations (rv_evaluate, rv_evaluate_batch; the streaming evaluator once per chunk) ran each schedule:
 * out[0] = one launch per dependency level, out[1] = one workgroup per slice of witness words walking every level (csrc/eval.hip).
 * The results are the same either way. */
int rv_hook_eval_schedules(uint64_t out[2]);
/* Running totals since process start, counted where the provers and the evaluator queue the copies (the streams do not
 * count): out[0] = witness bytes copied host-to-device, out[1] = witness bytes taken from device memory (copied
 * device-to-device, or read in place by the evaluator), out[2] = evaluation result bytes copied device-to-host.  Only the elements
 * the Input ops consume are counted.  Calls refused before anything is launched count nothing. */
int rv_hook_witness_traffic(uint64_t out[3]);
/* The streams' own running totals since process start, counted where they queue their copies: out[0] = witness bytes sent
 * host-to-device, out[1] = witness bytes taken from device memory, out[2] = proof bytes copied device-to-host at finish, out[3] =
 * proof bytes copied host-to-device at a streaming verifier's begin.  A chunk served from kept transcripts copies no witness. */
int rv_hook_stream_traffic(uint64_t out[4]);
/* rv_stream_verify_begin_device / _begin_batch_device proofs of this process that took out[0] = the in-place path, out[1] = the host
 * fallback (calls refused with RV_E_ARG count as neither). */
int rv_hook_stream_verify_device_paths(uint64_t out[2]);
/* The streams' position-keyed witness digest of n_gf2 GF(2) bytes at input ordinal first_gf2 and n_z64 words at first_z64: *host_out
 * from the host loop, *dev_out from the kernel the device-witness feeds use, run on a device copy of the same arrays (the GF(2) copy
 * starts 3 bytes into its allocation).  They must agree on every input. */
int rv_hook_stream_wit_sums(rv_ctx *ctx, const uint8_t *gf2, size_t n_gf2, uint64_t first_gf2, const uint64_t *z64, size_t n_z64,
                            uint64_t first_z64, uint64_t *host_out, uint64_t *dev_out);
/* The early-corrections plan of a program (host only, no device): the ops are compiled as rv_circuit_compile_ex(flags) would and
 * the plan rv_prove would use is built and checked against the compiled gate records.  out[0] = a plan exists (0 / 1: the circuit
 * is pure GF(2) with >= 2^21 Mul gates -- RV_EARLY_MIN -- or pure Z64, its preprocessing rows complete in step with the levels
 * and fit the PCIe window), [1] = Z64 form, [2] = repetitions staged, [3] = chunks, [4] = staging bytes, [5] = 1 when no level
 * after a chunk's ready level writes one of its rows and the ready level itself does, [6 + k] = chunk k's ready level (k < 16).
 * Returns the compiler's status. */
int rv_hook_early_plan(const rv_op *ops, size_t n_ops, size_t z64_wires, size_t gf2_wires, uint32_t flags, uint64_t out[22]);

#ifdef __cplusplus
}
#endif
#endif /* REVERIE_AMD_H */
