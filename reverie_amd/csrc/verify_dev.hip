// see verify_dev.h
//
// k_parse_proof: one wavefront, whose first lane runs walk_proof -- at most 80 records, each a handful of dependent loads (a
// record's place follows from the lengths in front of it); a count that is not 40 / 216 stops the walk before it starts, so no
// byte string makes the GPU walk more than that.
// k_fill_slots_dev: the slot arrays from the table, the proof's keys, seeds and commitments copied byte by byte from the offsets
// the walk took (all of them inside the proof: VW_OK means every field of it was found).
#include "verify_dev.h"

#include "../../include/reverie_amd.h"

namespace rv {

namespace {

constexpr uint32_t R = RV_TOTAL_REPS, ON = RV_ONLINE_REPS;
static_assert(ON == VW_N_ON && R - ON == VW_N_PRE, "the table is laid out for 40 online and 216 preprocessing repetitions");
constexpr int FILL_TB = 256, FILL_GROUPS = 32;

__global__ __launch_bounds__(64) void k_parse_proof(const uint8_t* __restrict__ bytes, uint64_t len, int framing, const uint64_t* __restrict__ lens,
                                                    uint64_t* __restrict__ table, uint64_t* __restrict__ head_mapped) {
    if (threadIdx.x != 0) return;
    uint64_t l[4] = {0, 0, 0, 0};
    if (lens)
        for (int i = 0; i < 4; i++) l[i] = lens[i];
    const int status = walk_proof(bytes, len, framing, l, table);
    if (head_mapped) {
        // (a stopped walk leaves words unwritten: zeros for them.  The host reads the head once the stream has drained)
        head_mapped[0] = (uint64_t)status;
        for (int i = 1; i < VW_HEAD_WORDS; i++) head_mapped[i] = status == VW_OK ? table[VW_HEAD + i] : 0;
    }
}

// k_parse_proof for the proofs of a batch: block b's first lane walks proof b into tables[b] and leaves the tail -- status, omit
// bytes, comm -- in heads[b], a dense block of its own (device memory or mapped host memory: the host reads nothing else)
__global__ __launch_bounds__(64) void k_parse_proofs(const BatchProofRef* __restrict__ refs, uint64_t* __restrict__ tables,
                                                     uint64_t* __restrict__ heads) {
    if (threadIdx.x != 0) return;
    const BatchProofRef ref = refs[blockIdx.x];
    uint64_t* table = tables + (size_t)blockIdx.x * VW_WORDS;
    uint64_t* head = heads + (size_t)blockIdx.x * VW_HEAD_WORDS;
    const uint64_t l[4] = {0, 0, 0, 0};
    const int status = walk_proof(ref.bytes, ref.len, VW_FRAMING_PROOF, l, table);
    head[0] = (uint64_t)status;
    for (int i = 1; i < VW_HEAD_WORDS; i++) head[i] = status == VW_OK ? table[VW_HEAD + i] : 0;
}

// the slot arrays of one proof from its table (tid of nth threads)
__device__ __forceinline__ void fill_slots_body(const uint8_t* __restrict__ p, const uint64_t* __restrict__ t, int has64, const DevSlotArrays& a,
                                                uint32_t tid, uint32_t nth) {
    const uint8_t* om = (const uint8_t*)(t + VW_OMIT);
    const uint64_t pre2 = t[VW_PRE], pre64 = t[VW_PRE + 1];
    // per slot: omit (8: not opened) and the three vectors' places -- a GF(2) vector has the length of its group's first record,
    // a Z64 one its own, cut to the whole words of the first record's (fill_slots)
    for (uint32_t r = tid; r < R; r += nth) {
        const bool on = r < ON;
        const uint64_t* o = t + VW_REC + 8 * (on ? r : 0);
        const uint64_t* o0 = t + VW_REC + 8 * (on ? r & ~7u : 0);
        a.omit[r] = on ? om[r] : (uint8_t)8;
        a.src[0 * R + r] = on ? o[VW_OFF_REC] : 0;
        a.src[1 * R + r] = on ? o0[VW_LEN_REC] : 0;
        a.src[2 * R + r] = on ? o[VW_OFF_CORR] : 0;
        a.src[3 * R + r] = on ? o0[VW_LEN_CORR] : 0;
        a.src[4 * R + r] = on ? o[VW_OFF_IN] : 0;
        a.src[5 * R + r] = on ? o0[VW_LEN_IN] : 0;
        if (has64) {
            const uint64_t* z = o + 8 * ON;
            const uint64_t* z0 = o0 + 8 * ON;
            auto cut = [](uint64_t n, uint64_t first) { return n < first / 8 * 8 ? n : first / 8 * 8; };
            a.omit64[r] = on ? om[ON + r] : (uint8_t)8;
            a.src64[0 * R + r] = on ? z[VW_OFF_REC] : 0;
            a.src64[1 * R + r] = on ? cut(z[VW_LEN_REC], z0[VW_LEN_REC]) : 0;
            a.src64[2 * R + r] = on ? z[VW_OFF_CORR] : 0;
            a.src64[3 * R + r] = on ? cut(z[VW_LEN_CORR], z0[VW_LEN_CORR]) : 0;
            a.src64[4 * R + r] = on ? z[VW_OFF_IN] : 0;
            a.src64[5 * R + r] = on ? cut(z[VW_LEN_IN], z0[VW_LEN_IN]) : 0;
        }
    }
    // per quad word: the streams BatchGen keeps (all but the omitted player's) and which of its four repetitions are opened
    for (uint32_t q = tid; q < R / 4; q += nth) {
        uint32_t keep = 0xFFFFFFFFu, keep64 = 0xFFFFFFFFu, onm = 0;
        for (uint32_t i = 0; i < 4; i++) {
            const uint32_t r = 4 * q + i;
            if (r >= ON) continue;
            keep &= ~(1u << (31 - 8 * i - (om[r] & 7u)));  // (VW_OK: every omit byte is below 8)
            keep64 &= ~(1u << (31 - 8 * i - (om[ON + r] & 7u)));
            onm |= 0xFFu << (24 - 8 * i);
        }
        a.keep[q] = keep;
        a.onm[q] = onm;
        if (has64) a.keep64[q] = keep64;
    }
    // the preprocessing slots' seeds and the online commitments they carry over; the online slots' keys
    for (uint32_t i = tid; i < R * 16; i += nth) {
        const uint32_t r = i / 16, j = i % 16;
        a.seeds[i] = r < ON ? (uint8_t)0 : p[pre2 + (uint64_t)(r - ON) * 48 + j];
        if (has64) a.seeds64[i] = r < ON ? (uint8_t)0 : p[pre64 + (uint64_t)(r - ON) * 48 + j];
    }
    for (uint32_t i = tid; i < R * 32; i += nth) {
        const uint32_t r = i / 32, j = i % 32;
        a.hco[i] = r < ON ? (uint8_t)0 : p[pre2 + (uint64_t)(r - ON) * 48 + 16 + j];
        a.hco64[i] = r < ON ? (uint8_t)0 : p[pre64 + (uint64_t)(r - ON) * 48 + 16 + j];
    }
    for (uint32_t i = tid; i < R * 128; i += nth) {
        const uint32_t r = i / 128, j = i % 128;
        a.hkeys[i] = r < ON ? p[t[VW_REC + 8 * r + VW_KEYS] + j] : (uint8_t)0;
        if (has64) a.hkeys64[i] = r < ON ? p[t[VW_REC + 8 * (ON + r) + VW_KEYS] + j] : (uint8_t)0;
    }
}

__global__ __launch_bounds__(FILL_TB) void k_fill_slots_dev(const uint8_t* __restrict__ p, const uint64_t* __restrict__ t, int has64, DevSlotArrays a) {
    fill_slots_body(p, t, has64, a, blockIdx.x * FILL_TB + threadIdx.x, gridDim.x * FILL_TB);
}

// k_fill_slots_dev for the live proofs of a batch (gridDim.y): proof k's arrays go into its slot of the verifier's slab, at the
// offsets of L, and the opened quad words -- 0 .. 9, from the slot order alone -- into the slot's quads
__global__ __launch_bounds__(FILL_TB) void k_fill_slots_batch(const BatchProofRef* __restrict__ refs, uint8_t* __restrict__ slab, BatchSlotLayout L,
                                                              int has64) {
    const BatchProofRef ref = refs[blockIdx.y];
    uint8_t* d = slab + (size_t)blockIdx.y * L.stride;
    DevSlotArrays a{};
    a.seeds = d + L.seeds, a.omit = d + L.omit, a.hkeys = d + L.hkeys, a.hco = d + L.hco, a.hco64 = d + L.hco64;
    a.keep = (uint32_t*)(d + L.keep), a.onm = (uint32_t*)(d + L.onm), a.src = (uint64_t*)(d + L.src);
    a.seeds64 = d + L.seeds64, a.omit64 = d + L.omit64, a.hkeys64 = d + L.hkeys64;
    a.keep64 = (uint32_t*)(d + L.keep64), a.src64 = (uint64_t*)(d + L.src64);
    const uint32_t tid = blockIdx.x * FILL_TB + threadIdx.x, nth = gridDim.x * FILL_TB;
    fill_slots_body(ref.bytes, ref.table, has64, a, tid, nth);
    uint32_t* quads = (uint32_t*)(d + L.quads);
    for (uint32_t q = tid; q < R / 4; q += nth) quads[q] = q < ON / 4 ? q : 0u;
}

}  // namespace

void launch_parse_proof(hipStream_t st, const uint8_t* d_bytes, uint64_t len, int framing, const uint64_t* d_lens, uint64_t* d_table,
                        uint64_t* head_mapped) {
    hipLaunchKernelGGL(k_parse_proof, dim3(1), dim3(64), 0, st, d_bytes, len, framing, d_lens, d_table, head_mapped);
}

void launch_fill_slots_dev(hipStream_t st, const uint8_t* d_bytes, const uint64_t* d_table, bool has64, const DevSlotArrays& a) {
    hipLaunchKernelGGL(k_fill_slots_dev, dim3(FILL_GROUPS), dim3(FILL_TB), 0, st, d_bytes, d_table, has64 ? 1 : 0, a);
}

void launch_parse_proofs(hipStream_t st, const BatchProofRef* d_refs, uint32_t batch, uint64_t* d_tables, uint64_t* heads) {
    hipLaunchKernelGGL(k_parse_proofs, dim3(batch), dim3(64), 0, st, d_refs, d_tables, heads);
}

void launch_fill_slots_batch(hipStream_t st, const BatchProofRef* d_refs, uint32_t n_live, uint8_t* d_slab, const BatchSlotLayout& L, bool has64) {
    constexpr int GROUPS = 8;  // (a proof's share of the grid: 256 proofs fill the chip many times over)
    hipLaunchKernelGGL(k_fill_slots_batch, dim3(GROUPS, n_live), dim3(FILL_TB), 0, st, d_refs, d_slab, L, has64 ? 1 : 0);
}

}  // namespace rv

// Test hook (host only, no device): walk_proof over bytes[0, len) into table[VW_WORDS]; framing 0 = bincode(Proof), 1 = the four
// sections, whose lengths the caller leaves in table[0 .. 3] (their sum must be len).  *status: what the walk ended with.
extern "C" int rv_hook_verify_walk(const uint8_t* bytes, size_t len, int framing, uint64_t* table, int* status) {
    if ((len && !bytes) || !table || !status || (framing != rv::VW_FRAMING_PROOF && framing != rv::VW_FRAMING_SECTIONS)) return RV_E_ARG;
    uint64_t lens[4] = {0, 0, 0, 0};
    if (framing == rv::VW_FRAMING_SECTIONS) {
        uint64_t sum = 0;
        for (int i = 0; i < 4; i++) {
            lens[i] = table[i];
            if (lens[i] > (uint64_t)len - sum) return RV_E_ARG;
            sum += lens[i];
        }
        if (sum != (uint64_t)len) return RV_E_ARG;
    }
    for (int i = 0; i < rv::VW_WORDS; i++) table[i] = 0;
    *status = rv::walk_proof(bytes, (uint64_t)len, framing, lens, table);
    return RV_OK;
}
