// The GF(2) level interpreter for gfx950: one launch per dependency level, and runs of narrow levels in one workgroup.
//
// Replaces (all under the reference's src/):
//   interpreter/single.rs:25-157      Instance::step / op_mul over the GF(2) ring
//   algebra/gf2/domain.rs:10-63       Share*Recon, reconstruct (per-byte parity)
//   transcript/prover.rs:181-232      ProverTranscript::{input,reconstruct,correction,zero_check}
//   transcript/verifier/online.rs:122-183, verifier/preprocess.rs:46-79
// (transcript hashing: b3_tree.hip; Fiat-Shamir and the openings: open.hip)
//
// Lane mapping: one lane = one quad word = 4 repetitions x 8 players (see internal.h);
// NQ consecutive lanes cover every repetition of the shard for one gate, so a wavefront
// reads/writes whole 256-byte rows.  Gates of one dependency level are independent and
// are spread over the grid; levels are separate launches.
#include <stdlib.h>

#include <algorithm>
#include <atomic>

#include "gf2dev.h"
#include "internal.h"
#include "launch.h"

namespace rv {

static size_t g_device_lds_limit = 160 * 1024;
void set_device_lds_limit(size_t bytes) { g_device_lds_limit = bytes; }
size_t device_lds_limit() { return g_device_lds_limit; }

static std::atomic<uint64_t> g_interp_launches[IX_COUNT][4];
void count_interp_launch(int exec, int mode) {
    const int col = mode == MODE_PROVE ? 0 : mode == MODE_PROVE_V ? 1 : mode == MODE_VERIFY ? 2 : 3;
    g_interp_launches[exec][col].fetch_add(1, std::memory_order_relaxed);
}
void interp_launch_counts(uint64_t out[][4], bool reset) {
    for (int e = 0; e < IX_COUNT; e++)
        for (int m = 0; m < 4; m++)
            out[e][m] = reset ? g_interp_launches[e][m].exchange(0, std::memory_order_relaxed) : g_interp_launches[e][m].load(std::memory_order_relaxed);
}


// XOR of the n listed base rows / their corr bits.  Unused slots hold the zero row, so all
// RV_LIN_K slots are loaded unconditionally with STATIC indices (a runtime-indexed id array would
// push the gate record into scratch memory; a per-slot branch would serialise the loads).
__device__ __forceinline__ uint32_t gather_rows(const uint32_t* rows, const uint32_t* ids, uint32_t NQ, uint32_t q) {
    uint32_t v = 0;
#pragma unroll
    for (int i = 0; i < RV_LIN_K; i++) v ^= rows[(size_t)ids[i] * NQ + q];
    return v;
}
__device__ __forceinline__ uint32_t gather_corr_byte(const uint8_t* corr, const uint32_t* ids, uint32_t NQ, uint32_t o) {
    uint32_t v = 0;
#pragma unroll
    for (int i = 0; i < RV_LIN_K; i++) v ^= corr[(size_t)ids[i] * (NQ >> 1) + o];
    return v;
}
__device__ __forceinline__ uint32_t gather_corr(const uint8_t* corr, const uint32_t* ids, uint32_t NQ, uint32_t q) {
    return (gather_corr_byte(corr, ids, NQ, q >> 1) >> (4 * (q & 1))) & 0xFu;
}

// MODE_PROVE_V: cleartext value of an operand = XOR of its base rows' values (unused slots hold the zero row, value 0)
__device__ __forceinline__ uint32_t gather_vclr(const uint8_t* vclr, const uint32_t* ids) {
    uint32_t v = 0;
#pragma unroll
    for (int i = 0; i < RV_LIN_K; i++) v ^= vclr[ids[i]];
    return v;
}

// MODE_VERIFY_C (round 4): the verifier of a whole proof without corr rows.  Only the opened repetitions need public
// corrections, and in the verifier's slot order they sit in the first sixteen quad words of a row: ONE u64 per row (nibble q =
// the four corr bits of quad word q, the 32-byte row's own bit order) instead of a 32-byte row that every lane gathers a byte
// of.  An operand's corrections are then one 8-byte access at a wave-uniform address per base row, an XOR gate's are a u64 XOR
// by one lane, and lazy linear forms stop costing the verifier a row access per base.
__device__ __forceinline__ uint32_t vc_nib(uint64_t c, uint32_t q) {
    const uint32_t w = (q & 8) ? (uint32_t)(c >> 32) : (uint32_t)c;
    return q < 16 ? (w >> (4 * (q & 7))) & 0xFu : 0u;
}
__device__ __forceinline__ uint64_t gather_vc(const uint64_t* vc, const uint32_t* ids) {
    uint64_t v = 0;
#pragma unroll
    for (int i = 0; i < RV_LIN_K; i++) v ^= vc[ids[i]];
    return v;
}
// the lanes q = 0 .. 15 of a full-width row (one DPP row) put their nibbles together: lanes 7 and 15 end up with the low and
// the high word (OR over the eight lanes before them) and store it
__device__ __forceinline__ void vc_store(uint64_t* vc, size_t row, uint32_t q, uint32_t smeared) {
    uint32_t v = q < 16 ? compress4(smeared) << (4 * (q & 7)) : 0u;
    v |= (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x111, 0xF, 0xF, true);  // row_shr:1
    v |= (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x112, 0xF, 0xF, true);  // row_shr:2
    v |= (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x114, 0xF, 0xF, true);  // row_shr:4
    if (q == 7 || q == 15) ((uint32_t*)(vc + row))[q >> 3] = v;
}
constexpr bool is_verify(int mode) { return mode == MODE_VERIFY || mode == MODE_VERIFY_C; }

template <int MODE>
__device__ __forceinline__ void interp_one(const Gate& g, const InterpParams& p, uint32_t NQ, uint32_t q, uint32_t onm) {
    switch (g_op(g)) {
    case G_INPUT: {
        const uint32_t lam = p.rows[(size_t)g.m * NQ + q];
        uint32_t corr;
        if (!is_verify(MODE)) {
            const uint32_t w = p.wit[g.x] ? 0xFFFFFFFFu : 0u;
            corr = w ^ recon32(lam);
        } else {
            corr = onm ? (p.sup_in[(size_t)g.x * p.sup_nq + q] & onm) : 0u;  // (rows of quads without an opened repetition are never written)
        }
        if (!is_verify(MODE) || onm) p.on[(size_t)g.eo * NQ + q] = corr;
        if (MODE == MODE_PROVE_V) {
            if (q == 0) p.vclr[g.dst] = p.wit[g.x] ? 1 : 0;
        } else if (MODE == MODE_VERIFY_C) {
            vc_store(p.vc, g.dst, q, corr);
        } else {
            store_bits(p.corr, g.dst, NQ, q, corr);
        }
        break;
    }
    case G_XORK: {
        p.rows[(size_t)g.dst * NQ + q] = gather_rows(p.rows, g.a, NQ, q) ^ gather_rows(p.rows, g.b, NQ, q);
        if (MODE == MODE_PROVE_V) {
            if (q == 0) p.vclr[g.dst] = (uint8_t)((g_ca(g) ^ gather_vclr(p.vclr, g.a) ^ gather_vclr(p.vclr, g.b)) & 1u);
            break;
        }
        if (MODE == MODE_VERIFY_C) {
            if (q == 0) p.vc[g.dst] = gather_vc(p.vc, g.a) ^ gather_vc(p.vc, g.b) ^ (g_ca(g) ? ~0ull : 0ull);
            break;
        }
        // corr bits: plain byte XOR, no expansion needed
        if (!(q & 1)) {
            const size_t h = NQ >> 1, o = q >> 1;
            const uint32_t c = (g_ca(g) ? 0xFFu : 0u) ^ gather_corr_byte(p.corr, g.a, NQ, o) ^ gather_corr_byte(p.corr, g.b, NQ, o);
            p.corr[(size_t)g.dst * h + o] = (uint8_t)c;
        }
        break;
    }
    case G_RANDOM: {
        if (MODE == MODE_VERIFY_C) {
            if (q == 0) p.vc[g.dst] = 0;
            break;
        }
        if (!(q & 1)) p.corr[(size_t)g.dst * (NQ >> 1) + (q >> 1)] = 0;
        break;
    }
    case G_MUL: {
        const uint32_t lx = gather_rows(p.rows, g.a, NQ, q), ly = gather_rows(p.rows, g.b, NQ, q);
        const uint32_t lab = p.rows[(size_t)g.m * NQ + q], lnew = p.rows[(size_t)(g.m + 1) * NQ + q];
        const uint32_t a = recon32(lx), b = recon32(ly), c = recon32(lab);
        uint32_t cx, cy, vx = 0, vy = 0;
        if (MODE == MODE_PROVE_V) {
            vx = (gather_vclr(p.vclr, g.a) ^ g_ca(g)) & 1u;
            vy = (gather_vclr(p.vclr, g.b) ^ g_cb(g)) & 1u;
            cx = a ^ (vx ? 0xFFFFFFFFu : 0u);  // corr = value - reconstruct(mask)
            cy = b ^ (vy ? 0xFFFFFFFFu : 0u);
        } else if (MODE == MODE_VERIFY_C) {
            cx = expand4(vc_nib(gather_vc(p.vc, g.a), q)) ^ (g_ca(g) ? 0xFFFFFFFFu : 0u);
            cy = expand4(vc_nib(gather_vc(p.vc, g.b), q)) ^ (g_cb(g) ? 0xFFFFFFFFu : 0u);
        } else {
            cx = expand4(gather_corr(p.corr, g.a, NQ, q)) ^ (g_ca(g) ? 0xFFFFFFFFu : 0u);
            cy = expand4(gather_corr(p.corr, g.b, NQ, q)) ^ (g_cb(g) ? 0xFFFFFFFFu : 0u);
        }
        uint32_t delta = (a & b) ^ c;
        uint32_t s = (ly & cx) ^ (lx & cy) ^ lab ^ lnew;
        uint32_t r;
        if (!is_verify(MODE)) {
            r = recon32(s);
        } else {
            // online-verified reps: supplied correction, add the unopened player's broadcast
            if (onm) {
                delta = (p.sup_corr[(size_t)g.ep * p.sup_nq + q] & onm) | (delta & ~onm);
                s ^= p.sup_rec[(size_t)g.x * p.sup_nq + q];
            }
            r = recon32(s) & onm;  // preprocessing-verified reps: reconstruct() returns zero
        }
        // verifier: the online transcript is only hashed for quads that hold an opened repetition (the other
        // repetitions' online digests come from the proof), so only those lanes store -- in the verifier's slot order
        // they are the first ten quads of a row, two 32-byte sectors instead of eight
        if (!is_verify(MODE) || onm) p.on[(size_t)g.eo * NQ + q] = s;
        store_bits(p.pre, g.ep, NQ, q, delta);
        if (MODE == MODE_PROVE_V) {
            if (q == 0) p.vclr[g.dst] = (uint8_t)(vx & vy);
        } else if (MODE == MODE_VERIFY_C) {
            vc_store(p.vc, g.dst, q, r ^ delta ^ (cx & cy));
        } else {
            store_bits(p.corr, g.dst, NQ, q, r ^ delta ^ (cx & cy));
        }
        break;
    }
    case G_RECON: {
        // B2A's recorded reconstruction (combine.rs:181-183): value = reconstruct(mask) + corr
        uint32_t m = gather_rows(p.rows, g.a, NQ, q);
        if (is_verify(MODE) && onm) m ^= p.sup_rec[(size_t)g.x * p.sup_nq + q];
        if (MODE == MODE_PROVE || onm) p.on[(size_t)g.eo * NQ + q] = m;
        uint32_t r = recon32(m);
        if (is_verify(MODE)) r &= onm;
        const uint32_t cx = expand4(gather_corr(p.corr, g.a, NQ, q)) ^ (g_ca(g) ? 0xFFFFFFFFu : 0u);
        p.rows[(size_t)g.dst * NQ + q] = 0;
        store_bits(p.corr, g.dst, NQ, q, r ^ cx);
        break;
    }
    case G_ASSERT: {
        uint32_t m = gather_rows(p.rows, g.a, NQ, q);
        if (is_verify(MODE) && onm) m ^= p.sup_rec[(size_t)g.x * p.sup_nq + q];
        if (!is_verify(MODE) || onm) p.on[(size_t)g.eo * NQ + q] = m;
        if (MODE == MODE_PROVE_V) {
            // the wire's value itself must be zero (prover.rs:221-228), the same in every repetition
            if (q == 0 && ((gather_vclr(p.vclr, g.a) ^ g_ca(g)) & 1u) != 0) atomicOr(p.err, RV_E_WITNESS_INVALID);
        } else {
            const uint32_t cx = expand4(MODE == MODE_VERIFY_C ? vc_nib(gather_vc(p.vc, g.a), q) : gather_corr(p.corr, g.a, NQ, q)) ^ (g_ca(g) ? 0xFFFFFFFFu : 0u);
            if (MODE == MODE_PROVE) {
                if ((recon32(m) ^ cx) != 0) atomicOr(p.err, RV_E_WITNESS_INVALID);
            } else {
                // online.rs:175-177: okay &= recon.is_zero() -- the reference never reads it; RV_VERIFY_STRICT does
                if (((recon32(m) ^ cx) & onm) != 0) atomicOr(p.err, RV_DEV_ZERO_CHECK);
            }
        }
        break;
    }
    default:
        break;
    }
}

template <int MODE>
__global__ __launch_bounds__(256) void k_interp(const Gate* __restrict__ gates, uint32_t lo, uint32_t hi, InterpParams p) {
    const uint32_t NQ = p.NQ;
    const uint32_t tid = blockIdx.x * blockDim.x + threadIdx.x;
    const uint32_t q = tid % NQ;
    const uint32_t worker = tid / NQ;
    const uint32_t n_workers = (gridDim.x * blockDim.x) / NQ;
    const uint32_t onm = (is_verify(MODE)) ? p.on_mask[q] : 0u;
    for (uint32_t gi = lo + worker; gi < hi; gi += n_workers) {
        const Gate g = gates[gi];
        interp_one<MODE>(g, p, NQ, q, onm);
    }
}

#ifndef RV_INTERP_UNROLL
#define RV_INTERP_UNROLL 4
#endif
#ifndef RV_INTERP_UNROLL_SMALL
#define RV_INTERP_UNROLL_SMALL 2
#endif
// gates a wavefront keeps in flight per step and gate group: narrow rows (small repetition shards, several gates per
// wavefront already) want fewer -- measured per rank on the 10^7-gate circuit: 128 repetitions (NQ = 32) 1.75 ms
// with 2, 1.64 with 4; 64 repetitions the same either way; 32 repetitions 1.02 with 2, 1.09 with 4
#ifndef RV_INTERP_UNROLL_MID
#define RV_INTERP_UNROLL_MID 4
#endif
#ifndef RV_INTERP_UNROLL_FAST
#define RV_INTERP_UNROLL_FAST 4
#endif
// two-row Xor steps of the full-width variant without the multi-base loops when they differ from its Mul steps (0 = the same).
// The point of unequal steps: a level's wave-steps against the wavefronts the chip holds at once -- a level that needs 1.4
// generations of wavefronts takes two rounds of memory latency, one that fits takes one
#ifndef RV_INTERP_UXOR_FAST
#define RV_INTERP_UXOR_FAST 0
#endif
// `general` = the kernel variant that also carries the multi-base Mul / Xor loops (more registers)
__host__ __device__ constexpr int interp_unroll(int NQ, bool general = true) {
    return NQ >= 64 ? (general ? RV_INTERP_UNROLL : RV_INTERP_UNROLL_FAST) : NQ >= 32 ? RV_INTERP_UNROLL_MID : RV_INTERP_UNROLL_SMALL;
}

// Gate-record prefetch.  A wavefront of a level launch lives for three dependent memory round trips: its gate records
// -> the operand rows they name -> the stores.  The records are static and contiguous (sorted by level, class), so
// the wavefront that runs unrolled step t also touches the records of step t + dist (one load instruction, a lane per
// 128-byte line, result unused), issued right behind its own row loads: by the time a later wavefront asks for them
// they sit in L2 and the first round trip is an L2 hit instead of an HBM miss.  Steps past the end of this level map
// onto the first steps of the next one (the gate array is contiguous across levels).  L2 is per XCD and workgroups
// are dealt to the XCDs round-robin, so producer and consumer must agree modulo 8 workgroups = 32 wavefronts: step t
// runs on wavefront t mod n_waves, and dist and the wrap-around are kept multiples of 32.
struct PfPlan {
    uint32_t dist;         // 0 = off
    uint32_t rem;          // steps of this level modulo 32 (added back after the wrap so that t' = t + dist - 32k)
    uint32_t n[2][4];      // [0] this level, [1] the next one: full unrolled steps of classes 0..3
    uint32_t start[2][4];  // first gate of each class
};
template <uint32_t STEP>
__device__ __forceinline__ const Gate* pf_target(const Gate* __restrict__ gates, const PfPlan& pf, uint32_t t) {
    uint32_t tt = t + pf.dist;
#pragma unroll
    for (int k = 0; k < 2; k++) {
#pragma unroll
        for (int c = 0; c < 4; c++) {
            if (tt < pf.n[k][c]) return gates + pf.start[k][c] + tt * STEP;
            tt -= pf.n[k][c];
        }
        tt += pf.rem;
    }
    return nullptr;
}
// one lane per 128-byte line of the STEP records at `g` (+ one for the unaligned tail); wave-uniform `g`.  The value
// is a plain load that pf_sink() "uses" after the wavefront's last store, so the compiler's own vmcnt bookkeeping
// covers it and its destination register stays reserved until it has landed.
template <uint32_t STEP>
__device__ __forceinline__ uint32_t pf_touch(const Gate* g, uint32_t lane) {
    constexpr uint32_t BYTES = STEP * (uint32_t)sizeof(Gate), NL = (BYTES + 127) / 128;
    uint32_t v = 0;
    if (g && lane <= NL) v = *(const uint32_t*)((const char*)g + (lane < NL ? lane * 128 : BYTES - 4));
    return v;
}
__device__ __forceinline__ void pf_sink(uint32_t v) { asm volatile("" ::"v"(v)); }

// Fast path (NQ = 64, 32, 16 or 8, i.e. R = 256 .. 32): a wavefront covers 64/NQ gates at a time and the
// per-class ranges run as 4-way unrolled loops that put every operand row of 4 x 64/NQ gates in flight
// before the first use — the generic kernel above is latency-bound on the dependent
// gate-record -> operand-row chain (2 HBM round trips per gate).  With NQ = 64 the gate index is
// wave-uniform and the records come through scalar loads.  KA / KB = operand base rows actually
// loaded per gate: exact for the common one-base-per-operand class, RV_LIN_K (unused slots point at
// the L1-hot zero row) for the rest.
template <int MODE, int NQ, int U, int KA, int KB>
__device__ __forceinline__ void mulU(const Gate* __restrict__ gates, uint32_t g0, const InterpParams& p, uint32_t sub, uint32_t q,
                                     uint32_t onm, const Gate* pf = nullptr) {
    constexpr uint32_t GPW = 64 / NQ, H = NQ / 2;
    // verifier: the online rows are stored in whole 32-byte sectors (the quads of the opened repetitions are a sector and a
    // quarter in its slot order, and a partially written sector is a read-modify-write at the memory side; the digests read
    // the opened quads only, so what the others hold does not matter)
    const bool on_wr = !is_verify(MODE) || ((__ballot(onm != 0) >> ((sub * NQ + q) & ~7u)) & 0xFFull) != 0;
    Gate g[U];
#pragma unroll
    for (int u = 0; u < U; u++) g[u] = gates[g0 + u * GPW + sub];
    uint32_t lx[U], ly[U], lab[U], lnew[U], bx[U], by[U], sc[U], sr[U];
    // slots >= 1 are loaded only when the operand really has that many bases (a wave-uniform branch at
    // NQ = 64); every load is issued before any value is used
    uint32_t ra[U][KA], ca[U][KA], rb[U][KB], cb[U][KB];
    // MODE_VERIFY_C: a lane reads the 32-bit half of a row's corrections word that holds its quad word's nibble (lanes 8 .. 15 the
    // high one; lanes >= 16 read the low one and use nothing of it)
    const uint32_t* const vc32 = (const uint32_t*)p.vc + ((q >> 3) & 1u);
#pragma unroll
    for (int u = 0; u < U; u++) {
        const int na = (int)g_na(g[u]), nb = (int)g_nb(g[u]);
#pragma unroll
        for (int i = 0; i < KA; i++) {
            ra[u][i] = 0;
            ca[u][i] = 0;
            if (i == 0 || i < na) {
                ra[u][i] = p.rows[(size_t)g[u].a[i] * NQ + q];
                ca[u][i] = MODE == MODE_VERIFY_C ? vc32[2 * (size_t)g[u].a[i]]
                                                 : MODE == MODE_PROVE_V ? p.vclr[g[u].a[i]] : p.corr[(size_t)g[u].a[i] * H + (q >> 1)];
            }
        }
#pragma unroll
        for (int i = 0; i < KB; i++) {
            rb[u][i] = 0;
            cb[u][i] = 0;
            if (i == 0 || i < nb) {
                rb[u][i] = p.rows[(size_t)g[u].b[i] * NQ + q];
                cb[u][i] = MODE == MODE_VERIFY_C ? vc32[2 * (size_t)g[u].b[i]]
                                                 : MODE == MODE_PROVE_V ? p.vclr[g[u].b[i]] : p.corr[(size_t)g[u].b[i] * H + (q >> 1)];
            }
        }
        // lambda_ab is read exactly once and the online row is not read again before the hash phase: nontemporal, so
        // they do not displace operand rows from L2 (interpreter 2.35 -> 2.30 ms; lambda_new -- the output wire's mask,
        // an operand of the next level -- and the XOR outputs are better left as plain accesses: 2.35 / 2.38)
        lab[u] = __builtin_nontemporal_load(&p.rows[(size_t)g[u].m * NQ + q]);
        lnew[u] = p.rows[(size_t)(g[u].m + 1) * NQ + q];
        if (is_verify(MODE)) {
            sc[u] = sr[u] = 0;
            if (onm) {  // supplied values exist (and are stored) only for quads with an opened repetition
                sc[u] = p.sup_corr[(size_t)g[u].ep * p.sup_nq + q];
                sr[u] = p.sup_rec[(size_t)g[u].x * p.sup_nq + q];
            }
        }
    }
    const uint32_t pfv = pf_touch<U * GPW>(pf, sub * NQ + q);
#pragma unroll
    for (int u = 0; u < U; u++) {
        lx[u] = ra[u][0];
        bx[u] = ca[u][0];
        ly[u] = rb[u][0];
        by[u] = cb[u][0];
#pragma unroll
        for (int i = 1; i < KA; i++) {
            lx[u] ^= ra[u][i];
            bx[u] ^= ca[u][i];
        }
#pragma unroll
        for (int i = 1; i < KB; i++) {
            ly[u] ^= rb[u][i];
            by[u] ^= cb[u][i];
        }
    }
#pragma unroll
    for (int u = 0; u < U; u++) {
        const uint32_t a = recon32(lx[u]), b = recon32(ly[u]), c = recon32(lab[u]);
        uint32_t cx, cy;
        const uint32_t vx = (bx[u] ^ g_ca(g[u])) & 1u, vy = (by[u] ^ g_cb(g[u])) & 1u;  // MODE_PROVE_V: the operands' cleartext values
        if (MODE == MODE_PROVE_V) {
            cx = a ^ (vx ? 0xFFFFFFFFu : 0u);  // corr = value - reconstruct(mask)
            cy = b ^ (vy ? 0xFFFFFFFFu : 0u);
        } else if (MODE == MODE_VERIFY_C) {
            cx = expand4(q < 16 ? (bx[u] >> (4 * (q & 7))) & 0xFu : 0u) ^ (g_ca(g[u]) ? 0xFFFFFFFFu : 0u);
            cy = expand4(q < 16 ? (by[u] >> (4 * (q & 7))) & 0xFu : 0u) ^ (g_cb(g[u]) ? 0xFFFFFFFFu : 0u);
        } else {
            cx = expand4((bx[u] >> (4 * (q & 1))) & 0xFu) ^ (g_ca(g[u]) ? 0xFFFFFFFFu : 0u);
            cy = expand4((by[u] >> (4 * (q & 1))) & 0xFu) ^ (g_cb(g[u]) ? 0xFFFFFFFFu : 0u);
        }
        uint32_t delta = (a & b) ^ c;
        uint32_t s = (ly[u] & cx) ^ (lx[u] & cy) ^ lab[u] ^ lnew[u];
        uint32_t r = 0;
        if (MODE == MODE_PROVE) {
            r = recon32(s);
        } else if (is_verify(MODE)) {
            delta = (sc[u] & onm) | (delta & ~onm);
            s ^= sr[u];
            r = recon32(s) & onm;
        }
        if (!is_verify(MODE) || on_wr) __builtin_nontemporal_store(s, &p.on[(size_t)g[u].eo * NQ + q]);
        store_bits(p.pre, g[u].ep, NQ, q, delta);
        if (MODE == MODE_PROVE_V) {
            if (q == 0) p.vclr[g[u].dst] = (uint8_t)(vx & vy);
        } else if (MODE == MODE_VERIFY_C) {
            vc_store(p.vc, g[u].dst, q, r ^ delta ^ (cx & cy));
        } else {
            store_bits(p.corr, g[u].dst, NQ, q, r ^ delta ^ (cx & cy));
        }
    }
    pf_sink(pfv);
}

// G_XORK: N = base rows loaded per gate (2: a[0], a[1]; 6: a[0..2], b[0..2] with zero-row padding)
template <int MODE, int NQ, int U, int N>
__device__ __forceinline__ void xorU(const Gate* __restrict__ gates, uint32_t g0, const InterpParams& p, uint32_t sub, uint32_t q,
                                     const Gate* pf = nullptr) {
    constexpr uint32_t GPW = 64 / NQ, H = NQ / 2;
    Gate g[U];
#pragma unroll
    for (int u = 0; u < U; u++) g[u] = gates[g0 + u * GPW + sub];
    uint32_t x[U], bx[U], rr[U][N], cc[U][N];
#pragma unroll
    for (int u = 0; u < U; u++) {
        const int na = (int)g_na(g[u]), nb = (int)g_nb(g[u]);
#pragma unroll
        for (int i = 0; i < N; i++) {
            const uint32_t id = (N == 2) ? g[u].a[i] : (i < RV_LIN_K ? g[u].a[i] : g[u].b[i - RV_LIN_K]);
            rr[u][i] = 0;
            cc[u][i] = 0;
            // only the slots the gate uses (N == 2: both by construction)
            if (N == 2 || (i < RV_LIN_K ? i < na : i - RV_LIN_K < nb)) {
                rr[u][i] = p.rows[(size_t)id * NQ + q];
                // H corr bytes per row: the first H lanes of the gate's lane group carry them (MODE_PROVE_V: one value byte)
                if (MODE == MODE_PROVE_V) {
                    if (q == 0) cc[u][i] = p.vclr[id];
                } else if (MODE == MODE_VERIFY_C) {
                    if (q < 2) cc[u][i] = ((const uint32_t*)p.vc)[2 * (size_t)id + q];  // (lanes 0, 1: the word's two halves)
                } else if (q < H) {
                    cc[u][i] = p.corr[(size_t)id * H + q];
                }
            }
        }
    }
    const uint32_t pfv = pf_touch<U * GPW>(pf, sub * NQ + q);
#pragma unroll
    for (int u = 0; u < U; u++) {
        x[u] = 0;
        bx[u] = 0;
#pragma unroll
        for (int i = 0; i < N; i++) {
            x[u] ^= rr[u][i];
            bx[u] ^= cc[u][i];
        }
    }
#pragma unroll
    for (int u = 0; u < U; u++) {
        p.rows[(size_t)g[u].dst * NQ + q] = x[u];
        if (MODE == MODE_PROVE_V) {
            if (q == 0) p.vclr[g[u].dst] = (uint8_t)((bx[u] ^ g_ca(g[u])) & 1u);
        } else if (MODE == MODE_VERIFY_C) {
            if (q < 2) ((uint32_t*)p.vc)[2 * (size_t)g[u].dst + q] = bx[u] ^ (g_ca(g[u]) ? 0xFFFFFFFFu : 0u);
        } else if (q < H) {
            p.corr[(size_t)g[u].dst * H + q] = (uint8_t)(bx[u] ^ (g_ca(g[u]) ? 0xFFu : 0u));
        }
    }
    pf_sink(pfv);
}

// One dependency level, class by class (LevelRange), executed by wavefronts `wave` of `n_waves`: shared by the
// one-launch-per-level kernel (all wavefronts of the grid) and the narrow-run kernel (the 16 wavefronts of one
// workgroup, gate records in LDS).  Work is dealt to the wavefronts round-robin ACROSS the
// classes (`slot` = wave-steps handed out so far) — a level of five gates in three classes must land on five
// different wavefronts, not three times on wave 0.  All gates that do not fill a 4-way unrolled step go through ONE
// loop at the end, so the big per-gate switch exists once in the instruction stream.
// GENERAL = false: the level has (next to) no multi-base Mul / Xor gates (LevelRange classes 1 and 3 — the case for
// a circuit compiled with one base per wire, e.g. the wide layered workload): their unrolled loops are compiled
// out, which keeps the kernel at 45 registers = 8 wavefronts per SIMD instead of 6; stray gates of those classes
// take the common per-gate loop.
// UXOR: unroll depth of the Xor classes when it differs from the Mul classes' (0 = the same) -- the single-workgroup
// kernel runs 8-gate Xor steps on circuits without multi-base gates
template <int MODE, int NQ, bool GENERAL = true, bool PF = false, int UXOR = 0>
__device__ __forceinline__ void run_level(const Gate* __restrict__ gates, const LevelRange& r, const InterpParams& p, uint32_t wave,
                                          uint32_t n_waves, uint32_t lane, uint32_t onm, const Gate* pf_gates = nullptr,
                                          const PfPlan* pf = nullptr) {
    constexpr uint32_t GPW = 64 / NQ;  // gates per wavefront per step
    const uint32_t q = lane % NQ, sub = lane / NQ;
    constexpr int U = interp_unroll(NQ, GENERAL);
    constexpr int UX = UXOR ? UXOR : U;
    static_assert(!PF || UX == U, "the prefetch plan assumes one step size");
    uint32_t slot = 0;
    auto my = [&](uint32_t used) { return (wave + n_waves - used % n_waves) % n_waves; };
    const uint32_t begin[5] = {r.lo, r.mul11, r.mul, r.xor2, r.xork}, end[5] = {r.mul11, r.mul, r.xor2, r.xork, r.hi};
    uint32_t rest[5];  // first gate of each class that is left to the common loop
#pragma unroll
    for (int c = 0; c < 4; c++) {
        // without the multi-base loops (GENERAL = false) the few gates of those classes all go to the common loop
        const uint32_t STEP = (uint32_t)(c >= 2 ? UX : U) * GPW;
        const uint32_t n_full = (!GENERAL && (c == 1 || c == 3)) ? 0u : (end[c] - begin[c]) / STEP;
        rest[c] = begin[c] + n_full * STEP;
        for (uint32_t g0 = begin[c] + my(slot) * STEP; g0 < rest[c]; g0 += n_waves * STEP) {
            const Gate* t = nullptr;
            if (PF && pf->dist) t = pf_target<U * GPW>(pf_gates, *pf, slot + (g0 - begin[c]) / STEP);
            if (c == 0) mulU<MODE, NQ, U, 1, 1>(gates, g0, p, sub, q, onm, t);               // G_MUL, one base per operand
            if (c == 1 && GENERAL) mulU<MODE, NQ, U, RV_LIN_K, RV_LIN_K>(gates, g0, p, sub, q, onm, t); // other G_MUL
            if (c == 2) xorU<MODE, NQ, UX, 2>(gates, g0, p, sub, q, t);                            // G_XORK of two bases
            if (c == 3 && GENERAL) xorU<MODE, NQ, UX, 2 * RV_LIN_K>(gates, g0, p, sub, q, t);                 // other G_XORK
        }
        slot += n_full;
    }
    rest[4] = begin[4];
    uint32_t cum[6];  // wave-steps (GPW gates each) of the common loop, per class
    cum[0] = 0;
#pragma unroll
    for (int c = 0; c < 5; c++) cum[c + 1] = cum[c] + (end[c] - rest[c] + GPW - 1) / GPW;
    for (uint32_t t = my(slot); t < cum[5]; t += n_waves) {
        uint32_t c0 = rest[0], e0 = end[0], base = 0;
#pragma unroll
        for (int c = 1; c < 5; c++)
            if (t >= cum[c]) c0 = rest[c], e0 = end[c], base = cum[c];
        const uint32_t gi = c0 + (t - base) * GPW + sub;
        if (gi < e0) interp_one<MODE>(gates[gi], p, NQ, q, onm);
    }
}

// (the full-width variant without the multi-base loops must fit eight wavefronts per SIMD: its verify-mode instance
// took 70 registers = seven; with the bound it is 61, without scratch.  Narrower rows keep the default: they would spill)
template <int MODE, int NQ, bool GENERAL>
__global__ __launch_bounds__(256, MODE == MODE_VERIFY_C ? (GENERAL ? 4 : 7) : (GENERAL || NQ != 64) ? 1 : 8) void k_interp_full(const Gate* __restrict__ gates, LevelRange r, InterpParams p, PfPlan pf) {
    // a level's wavefronts are short-lived and wait on memory most of the time; when the lane-distributed mask generator shares the
    // SIMD (api.hip: RV_OVERLAP) its two long-lived, always-ready wavefronts are the OLDEST and win every issue slot -- the level ran
    // 3.3x slower beside it until its own wavefronts asked for priority
    __builtin_amdgcn_s_setprio(1);
    const uint32_t lane = threadIdx.x & 63;
    const uint32_t wave = __builtin_amdgcn_readfirstlane((blockIdx.x * blockDim.x + threadIdx.x) >> 6);
    const uint32_t n_waves = gridDim.x * (blockDim.x >> 6);
    const uint32_t onm = (is_verify(MODE)) ? p.on_mask[lane % NQ] : 0u;
    // the rotation of run_level pays here too: a wavefront then runs ONE step of one class instead of a Mul step followed by an Xor step
    // (two generations of short-lived wavefronts beat one generation of twice-as-long ones: 2.52 -> 2.40 ms;
    // interleaving the two classes wave by wave instead of class after class is worse again, 2.56)
    constexpr int UXL = (!GENERAL && NQ == 64) ? RV_INTERP_UXOR_FAST : 0;
    constexpr bool PFL = UXL == 0 || UXL == interp_unroll(NQ, GENERAL);  // (the prefetch plan assumes one step size)
    run_level<MODE, NQ, GENERAL, PFL, UXL>(gates, r, p, wave, n_waves, lane, onm, gates, &pf);
}

// Batched proofs of one circuit (rv_prove_batch): blockIdx.y selects the proof; its buffers come from a device array
// of InterpParams.  The gate stream is shared, so one launch per level serves every proof in the batch.
template <int MODE, int NQ>
__global__ __launch_bounds__(256) void k_interp_full_b(const Gate* __restrict__ gates, LevelRange r, const InterpParams* __restrict__ pp) {
    const InterpParams p = pp[blockIdx.y];
    const uint32_t lane = threadIdx.x & 63;
    const uint32_t wave = __builtin_amdgcn_readfirstlane((blockIdx.x * blockDim.x + threadIdx.x) >> 6);
    const uint32_t n_waves = gridDim.x * (blockDim.x >> 6);
    const uint32_t onm = (is_verify(MODE)) ? p.on_mask[lane % NQ] : 0u;
    run_level<MODE, NQ>(gates, r, p, wave, n_waves, lane, onm);
}

// enough multi-base Mul / Xor gates in a level to be worth the variant with their unrolled loops?  (a handful
// -- constant operands in an otherwise one-base circuit -- run through the common per-gate loop instead)
static bool level_is_general(const LevelRange& r) { return (r.mul - r.mul11) + (r.xork - r.xor2) >= 64; }

// wavefronts that prefetch gate records look this many unrolled steps ahead: half a generation of resident
// wavefronts (8 per SIMD x 4 x 256 CUs = 8 192) measured best on full-width rows (interpreter 2.53 -> 2.42 ms on the
// 10^7-gate circuit; 2 048: 2.47, 8 192: 2.49, 16 384: 2.52).  Narrower rows (repetition shards) read their records
// through vector loads and gain nothing, so the default there is off.  RV_PF_DIST overrides (0 = off).
static uint32_t pf_dist(int NQ) {
    static const int env = [] {
        const char* e = getenv("RV_PF_DIST");
        return e ? atoi(e) : -1;
    }();
    const uint32_t v = env >= 0 ? (uint32_t)env : (NQ == 64 ? 4096u : 0u);
    return v & ~31u;
}

template <int NQ>
static PfPlan make_pf_plan(const LevelRange& r, const LevelRange* next) {
    constexpr uint32_t GPW = 64 / NQ;
    PfPlan pf{};
    pf.dist = pf_dist(NQ);
    if (!pf.dist) return pf;
    const LevelRange* lr[2] = {&r, next};
    uint32_t total = 0;
    for (int k = 0; k < 2; k++) {
        if (!lr[k]) break;
        const LevelRange& x = *lr[k];
        const bool general = level_is_general(x);
        const uint32_t step = (uint32_t)interp_unroll(NQ, general) * GPW;
        const uint32_t begin[4] = {x.lo, x.mul11, x.mul, x.xor2}, end[4] = {x.mul11, x.mul, x.xor2, x.xork};
        for (int c = 0; c < 4; c++) {
            pf.start[k][c] = begin[c];
            pf.n[k][c] = (!general && (c == 1 || c == 3)) ? 0u : (end[c] - begin[c]) / step;
            if (k == 0) total += pf.n[k][c];
        }
    }
    pf.rem = total & 31u;
    return pf;
}

template <int MODE, int NQ>
static void launch_interp_full_mode(hipStream_t st, dim3 grid, bool general, const Gate* d_gates, const LevelRange& r, const InterpParams& p,
                                    const PfPlan& pf) {
    count_interp_launch(general ? IX_FULL_GENERAL : IX_FULL_FAST, MODE);
    if (general)
        hipLaunchKernelGGL((k_interp_full<MODE, NQ, true>), grid, dim3(256), 0, st, d_gates, r, p, pf);
    else
        hipLaunchKernelGGL((k_interp_full<MODE, NQ, false>), grid, dim3(256), 0, st, d_gates, r, p, pf);
}

template <int NQ>
static void launch_interp_full(hipStream_t st, int mode, const Gate* d_gates, const LevelRange& r, const InterpParams& p,
                               const LevelRange* next) {
    constexpr uint32_t GPW = 64 / NQ;
    const bool general = level_is_general(r);
    const PfPlan pf = make_pf_plan<NQ>(r, next);
    const uint32_t u = (uint32_t)interp_unroll(NQ, general);
    uint64_t waves = ((uint64_t)(r.hi - r.lo) + u * GPW - 1) / (u * GPW);
    uint64_t blocks = (waves + 3) / 4;
    if (blocks > 4096) blocks = 4096;
    if (blocks < 1) blocks = 1;
    const dim3 grid((unsigned)blocks);
    if (mode == MODE_PROVE_V) return launch_interp_full_mode<MODE_PROVE_V, NQ>(st, grid, general, d_gates, r, p, pf);
    if (mode == MODE_PROVE) return launch_interp_full_mode<MODE_PROVE, NQ>(st, grid, general, d_gates, r, p, pf);
    if constexpr (NQ == 64)  // (MODE_VERIFY_C exists for full-width rows only; narrower rows verify with corr rows)
        if (mode == MODE_VERIFY_C) return launch_interp_full_mode<MODE_VERIFY_C, NQ>(st, grid, general, d_gates, r, p, pf);
    launch_interp_full_mode<MODE_VERIFY, NQ>(st, grid, general, d_gates, r, p, pf);
}

// (Rounds 2 and 4 built four more launch structures for the GF(2) prover -- persistent level kernels, the flat, split and chained
// schedules.  All byte-identical, all measured slower: DESIGN.md Appendix A; their last version is commit 56a26f2.)

// whether any level of the gate stream has enough multi-base gates for the kernel variants with their loops (the verifier's
// choice of MODE_VERIFY_C looks at it too)
bool any_level_general(const LevelRange* lr, size_t n_levels) {
    for (size_t l = 0; l < n_levels; l++)
        if (level_is_general(lr[l])) return true;
    return false;
}

// Narrow levels (deep circuits: ripple-carry adders, AES/SHA rounds) would be launch-bound at one
// kernel per level (~4.6 us each).  A run of consecutive narrow levels is executed by ONE 1024-thread
// workgroup instead: level -> __syncthreads() -> level ...; all waves share the CU's L1, so the
// workgroup-scope barrier is all the ordering the row/corr hand-off between levels needs.
// Per level the dependent chain used to be level_start[l+1] -> gate record -> operand rows (three L2 round trips,
// 1.57 us per level on SHA-256); the level table of the run and a rolling window of gate records now sit in LDS
// (filled by coalesced loads, one refill per NARROW_WIN gates), and a level runs through the same 4-way unrolled
// class loops as a full launch, so it costs one round trip per 64 gates plus the barrier.
// NQ = 0: generic row width (one gate per NQ lanes, no unrolling).
constexpr uint32_t NARROW_MAX_LEVELS = 1024;  // levels per launch (longer runs are split)
constexpr uint32_t NARROW_WIN = 1024;         // gate records resident in LDS (48 KiB) >= 2 x the widest narrow level
// LEAN: the run holds no multi-base Mul / Xor gates (a circuit compiled with one base per wire, e.g. AES-128): their
// unrolled loops are left out and the Xor steps take 8 gates -- a level of ~20 Mul + ~75 Xor gates is then 5 + 10 steps,
// one round of the 16 wavefronts instead of two (AES-128: 2.7 -> 2.6 us per level; a level moves ~100 KB through ONE CU,
// which at 64 B/clk is 0.7 us of the 2.6)
template <int MODE, int NQT, bool LEAN = false>
__device__ __forceinline__ void interp_narrow_body(const Gate* __restrict__ gates, const LevelRange* __restrict__ level_range,
                                                   uint32_t l0, uint32_t l1, const InterpParams& p) {
    __shared__ LevelRange s_lr[NARROW_MAX_LEVELS];
    __shared__ __attribute__((aligned(16))) Gate s_g[NARROW_WIN];
    const uint32_t NQ = NQT ? (uint32_t)NQT : p.NQ;
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint32_t onm = (is_verify(MODE)) ? p.on_mask[NQT ? lane % NQ : threadIdx.x % NQ] : 0u;
    const uint32_t n_lv = l1 - l0;
    {
        const uint32_t* src = (const uint32_t*)(level_range + l0);
        uint32_t* dst = (uint32_t*)s_lr;
        for (uint32_t i = threadIdx.x; i < n_lv * (uint32_t)(sizeof(LevelRange) / 4); i += 1024) dst[i] = src[i];
    }
    __syncthreads();
    const uint32_t g_end = s_lr[n_lv - 1].hi;
    uint32_t win_lo = s_lr[0].lo, win_hi = win_lo;  // gates [win_lo, win_hi) are in s_g
    for (uint32_t l = 0; l < n_lv; l++) {
        const LevelRange r = s_lr[l];
        if (r.hi > win_hi) {  // workgroup-uniform: the previous level's barrier has retired every reader of the old window
            win_lo = r.lo;
            win_hi = (r.lo + NARROW_WIN < g_end) ? r.lo + NARROW_WIN : g_end;
            const uint4* src = (const uint4*)(gates + win_lo);
            uint4* dst = (uint4*)s_g;
            for (uint32_t i = threadIdx.x; i < (win_hi - win_lo) * (uint32_t)(sizeof(Gate) / 16); i += 1024) dst[i] = src[i];
            __syncthreads();
        }
        const Gate* g = s_g - win_lo;  // indexed by absolute gate number
        if (NQT) {
            if (LEAN)
                run_level<MODE, NQT ? NQT : 64, false, false, 8>(g, r, p, wave, 16, lane, onm);
            else
                run_level<MODE, NQT ? NQT : 64>(g, r, p, wave, 16, lane, onm);
        } else {
            const uint32_t q = threadIdx.x % NQ, worker = threadIdx.x / NQ, n_workers = 1024 / NQ;
            for (uint32_t gi = r.lo + worker; gi < r.hi; gi += n_workers) interp_one<MODE>(g[gi], p, NQ, q, onm);
        }
        __syncthreads();
    }
}

template <int MODE, int NQT, bool LEAN = false>
__global__ __launch_bounds__(1024) void k_interp_narrow(const Gate* __restrict__ gates, const LevelRange* __restrict__ level_range,
                                                        uint32_t l0, uint32_t l1, InterpParams p) {
    interp_narrow_body<MODE, NQT, LEAN>(gates, level_range, l0, l1, p);
}
// batched proofs: one workgroup per proof (blockIdx.x), see k_interp_full_b
template <int MODE, int NQT>
__global__ __launch_bounds__(1024) void k_interp_narrow_b(const Gate* __restrict__ gates, const LevelRange* __restrict__ level_range,
                                                          uint32_t l0, uint32_t l1, const InterpParams* __restrict__ pp) {
    const InterpParams p = pp[blockIdx.x];
    interp_narrow_body<MODE, NQT>(gates, level_range, l0, l1, p);
}

template <int NQT, bool LEAN = false>
static void launch_narrow_nq(hipStream_t st, int mode, const Gate* d_gates, const LevelRange* d_lr, uint32_t a, uint32_t b,
                             const InterpParams& p) {
    count_interp_launch(NQT == 0 ? IX_NARROW_GATE : LEAN ? IX_NARROW_LEAN : IX_NARROW_CLASS, mode == MODE_PROVE ? MODE_PROVE : MODE_VERIFY);
    if (mode == MODE_PROVE)
        hipLaunchKernelGGL((k_interp_narrow<MODE_PROVE, NQT, LEAN>), dim3(1), dim3(1024), 0, st, d_gates, d_lr, a, b, p);
    else
        hipLaunchKernelGGL((k_interp_narrow<MODE_VERIFY, NQT, LEAN>), dim3(1), dim3(1024), 0, st, d_gates, d_lr, a, b, p);
}

void launch_interp_narrow(hipStream_t st, int mode, const Gate* d_gates, const LevelRange* d_level_range, uint32_t l0, uint32_t l1,
                          int tiny, const InterpParams& p) {
    for (uint32_t a = l0; a < l1; a += NARROW_MAX_LEVELS) {
        const uint32_t b = (a + NARROW_MAX_LEVELS < l1) ? a + NARROW_MAX_LEVELS : l1;
        // NQT = 0 is the plain per-gate loop (also the fallback for row widths without a class-loop instantiation)
        switch (tiny == 1 ? 0u : p.NQ) {
        case 64:
            if (tiny == 2)
                launch_narrow_nq<64, true>(st, mode, d_gates, d_level_range, a, b, p);
            else
                launch_narrow_nq<64>(st, mode, d_gates, d_level_range, a, b, p);
            break;
        case 32: launch_narrow_nq<32>(st, mode, d_gates, d_level_range, a, b, p); break;
        case 16: launch_narrow_nq<16>(st, mode, d_gates, d_level_range, a, b, p); break;
        case 8: launch_narrow_nq<8>(st, mode, d_gates, d_level_range, a, b, p); break;
        default: launch_narrow_nq<0>(st, mode, d_gates, d_level_range, a, b, p); break;
        }
    }
}

void launch_interp(hipStream_t st, int mode, const Gate* d_gates, const LevelRange& r, const InterpParams& p, const LevelRange* next) {
    if (r.hi <= r.lo) return;
    switch (p.NQ) {
    case 64: return launch_interp_full<64>(st, mode, d_gates, r, p, next);
    case 32: return launch_interp_full<32>(st, mode, d_gates, r, p, next);
    case 16: return launch_interp_full<16>(st, mode, d_gates, r, p, next);
    case 8: return launch_interp_full<8>(st, mode, d_gates, r, p, next);
    default: break;
    }
    const uint64_t want = (uint64_t)(r.hi - r.lo) * p.NQ;
    uint64_t blocks = (want + 255) / 256;
    if (blocks > 8192) blocks = 8192;
    count_interp_launch(IX_GENERIC, mode == MODE_PROVE ? MODE_PROVE : MODE_VERIFY);
    if (mode == MODE_PROVE)
        hipLaunchKernelGGL(k_interp<MODE_PROVE>, dim3((unsigned)blocks), dim3(256), 0, st, d_gates, r.lo, r.hi, p);
    else
        hipLaunchKernelGGL(k_interp<MODE_VERIFY>, dim3((unsigned)blocks), dim3(256), 0, st, d_gates, r.lo, r.hi, p);
}

// rv_prove_batch / rv_verify_batch: `batch` full proofs (256 repetitions, NQ = 64) of one circuit
void launch_interp_batched(hipStream_t st, const Gate* d_gates, const LevelRange& r, const InterpParams* d_pp, uint32_t batch, int mode) {
    if (r.hi <= r.lo || !batch) return;
    uint64_t waves = ((uint64_t)(r.hi - r.lo) + RV_INTERP_UNROLL - 1) / RV_INTERP_UNROLL;
    uint64_t blocks = (waves + 3) / 4;
    const uint64_t cap = std::max<uint64_t>(4096 / batch, 1);
    if (blocks > cap) blocks = cap;
    count_interp_launch(IX_B_FULL, mode == MODE_PROVE ? MODE_PROVE : MODE_VERIFY);
    if (mode == MODE_PROVE)
        hipLaunchKernelGGL((k_interp_full_b<MODE_PROVE, 64>), dim3((unsigned)blocks, batch), dim3(256), 0, st, d_gates, r, d_pp);
    else
        hipLaunchKernelGGL((k_interp_full_b<MODE_VERIFY, 64>), dim3((unsigned)blocks, batch), dim3(256), 0, st, d_gates, r, d_pp);
}

void launch_interp_narrow_batched(hipStream_t st, const Gate* d_gates, const LevelRange* d_level_range, uint32_t l0, uint32_t l1,
                                  int tiny, const InterpParams* d_pp, uint32_t batch, int mode) {
    for (uint32_t a = l0; a < l1 && batch; a += NARROW_MAX_LEVELS) {
        const uint32_t b = (a + NARROW_MAX_LEVELS < l1) ? a + NARROW_MAX_LEVELS : l1;
        count_interp_launch(tiny == 1 ? IX_B_NARROW_GATE : IX_B_NARROW_CLASS, mode == MODE_PROVE ? MODE_PROVE : MODE_VERIFY);
        if (mode == MODE_PROVE) {
            if (tiny == 1)
                hipLaunchKernelGGL((k_interp_narrow_b<MODE_PROVE, 0>), dim3(batch), dim3(1024), 0, st, d_gates, d_level_range, a, b, d_pp);
            else
                hipLaunchKernelGGL((k_interp_narrow_b<MODE_PROVE, 64>), dim3(batch), dim3(1024), 0, st, d_gates, d_level_range, a, b, d_pp);
        } else {
            if (tiny == 1)
                hipLaunchKernelGGL((k_interp_narrow_b<MODE_VERIFY, 0>), dim3(batch), dim3(1024), 0, st, d_gates, d_level_range, a, b, d_pp);
            else
                hipLaunchKernelGGL((k_interp_narrow_b<MODE_VERIFY, 64>), dim3(batch), dim3(1024), 0, st, d_gates, d_level_range, a, b, d_pp);
        }
    }
}

}  // namespace rv
