// Part of api.hip (#included there, one translation unit): proof parsing, rv_verify_shard / rv_verify_finish / rv_verify_ex: Proof::verify (proof/mod.rs:224-307).

// ------------------------------------------------------------------------------------
// proof parsing (bincode 1.3 fixint, SURVEY A.6)
// ------------------------------------------------------------------------------------
namespace {
struct OnRec {
    uint8_t omit;
    size_t keys, rec, corr, in;  // offsets into the proof
    uint64_t n_rec, n_corr, n_in;
};
struct PreRec {
    size_t seed, comm_online;
};
struct Single {
    std::vector<OnRec> on;
    std::vector<PreRec> pre;
};
struct Parsed {
    Single gf2, z64;
};
struct Reader {
    const uint8_t* p;
    size_t len, pos = 0;
    bool bad = false;
    size_t take(uint64_t n) {
        if (bad || n > len - pos) {
            bad = true;
            return 0;
        }
        size_t at = pos;
        pos += (size_t)n;
        return at;
    }
    uint64_t u64() {
        size_t at = take(8);
        if (bad) return 0;
        uint64_t v = 0;
        for (int i = 0; i < 8; i++) v |= (uint64_t)p[at + i] << (8 * i);
        return v;
    }
};
bool parse_single(Reader& r, Single& s) {
    uint64_t n = r.u64();
    if (r.bad || n > (r.len - r.pos) / 153 + 1) return false;
    s.on.resize((size_t)n);
    for (auto& o : s.on) {
        size_t at = r.take(1);
        if (r.bad) return false;
        o.omit = r.p[at];
        o.keys = r.take(128);
        o.n_rec = r.u64();
        o.rec = r.take(o.n_rec);
        o.n_corr = r.u64();
        o.corr = r.take(o.n_corr);
        o.n_in = r.u64();
        o.in = r.take(o.n_in);
        if (r.bad) return false;
    }
    n = r.u64();
    if (r.bad || n > (r.len - r.pos) / 48 + 1) return false;
    s.pre.resize((size_t)n);
    for (auto& q : s.pre) {
        q.seed = r.take(16);
        q.comm_online = r.take(32);
        if (r.bad) return false;
    }
    return true;
}
// returns RV_OK / RV_E_PROOF_MALFORMED; trailing bytes are ignored like bincode::deserialize_from (main.rs:101-103)
int parse_proof(const uint8_t* proof, size_t len, Parsed& out) {
    Reader r{proof, len};
    r.take(32);
    if (r.bad || !parse_single(r, out.gf2) || !parse_single(r, out.z64)) return RV_E_PROOF_MALFORMED;
    return RV_OK;
}
bool format_ok(const Parsed& p) {  // ProofSingle::check_format, proof/mod.rs:110-114
    return p.gf2.on.size() == RV_ONLINE_REPS && p.gf2.pre.size() == RV_PREPROCESSING_REPS &&
           p.z64.on.size() == RV_ONLINE_REPS && p.z64.pre.size() == RV_PREPROCESSING_REPS;
}

// ------------------------------------------------------------------------------------
// the verifier's slots (VerifierTranscriptOnline::new, online.rs:25-119; VerifierTranscriptPreprocess::new, preprocess.rs:17-43),
// shared by rv_verify_shard, rv_verify_batch and the streaming verifier.  Slots 0 .. 39 are the online records in proof order,
// 40 .. 255 the preprocessing ones.  They go by GROUPS of eight (group g = slots 8g .. 8g+7: 0 .. 4 online, 5 .. 31 preprocessing);
// a slot range starts and ends on a group.
// ------------------------------------------------------------------------------------
// The groups of a slot range [slot_begin, slot_begin + slot_count) (multiples of 8): the range forms below are calls of the
// group forms
std::vector<uint8_t> range_groups(uint32_t slot_begin, uint32_t slot_count) {
    std::vector<uint8_t> g(slot_count / 8);
    for (uint32_t k = 0; k < slot_count / 8; k++) g[k] = (uint8_t)(slot_begin / 8 + k);
    return g;
}
// what the online records of the groups groups[0 .. n_groups) must satisfy (a proof that passed format_ok):
// RV_OK / RV_E_PROOF_MALFORMED
int check_records(const Parsed& P, const uint8_t* groups, uint32_t n_groups) {
    for (uint32_t k = 0; k < n_groups; k++) {
        const uint32_t g0 = 8u * groups[k];
        if (g0 >= RV_ONLINE_REPS) continue;
        const OnRec* o = &P.gf2.on[g0];
        const OnRec* z = &P.z64.on[g0];
        for (int i = 0; i < 8; i++) {
            if (o[i].omit >= 8 || z[i].omit >= 8) return RV_E_PROOF_MALFORMED;  // UB upstream (gf2/share.rs:167-199)
            // Recon::unpack indexes every vector up to the first one's length (gf2/recon.rs:241-259)
            if (o[i].n_corr < o[0].n_corr || o[i].n_in < o[0].n_in) return RV_E_PROOF_MALFORMED;
            // Share::unpack_selected asserts equal lengths (gf2/share.rs:157-164)
            if (o[i].n_rec != o[0].n_rec) return RV_E_PROOF_MALFORMED;
        }
    }
    return RV_OK;
}
int check_records_range(const Parsed& P, uint32_t slot_begin, uint32_t slot_count) {
    const std::vector<uint8_t> g = range_groups(slot_begin, slot_count);
    return check_records(P, g.data(), (uint32_t)g.size());
}
// The proof bytes of an online group's eight records in one domain (they are adjacent in the proof): [begin, end)
struct Span {
    size_t begin, end;
};
Span group_span(const Single& s, uint32_t group) {
    const OnRec& a = s.on[8 * (size_t)group];
    const OnRec& b = s.on[8 * (size_t)group + 7];
    return {a.keys - 1, b.in + (size_t)b.n_in};  // (from the first record's omit byte to the last one's `in` vector)
}
// where fill_slots writes the arrays of R slots (NQ = R / 4 quad words)
struct SlotArrays {
    uint8_t *seeds, *omit, *hkeys, *hco, *hco64;  // [R][16], [R], [R][128], [R][32], [R][32]
    uint32_t *keep, *onm;                          // [NQ] each
    uint64_t* src;                                 // [6][R]: rec offset, length; corr offset, length; in offset, length
    uint8_t *seeds64, *omit64, *hkeys64;           // the Z64 side, as the GF(2) one
    uint32_t* keep64;
    uint64_t* src64;
};
// ... and host vectors for them
struct HostSlots {
    std::vector<uint8_t> seeds, omit, hkeys, hco, hco64, seeds64, omit64, hkeys64;
    std::vector<uint32_t> keep, onm, keep64;
    std::vector<uint64_t> src, src64;
    HostSlots(uint32_t R, bool has64)
        : seeds((size_t)R * 16), omit(R), hkeys((size_t)R * 128), hco((size_t)R * 32), hco64((size_t)R * 32), keep(R / 4), onm(R / 4),
          src((size_t)6 * R) {
        if (has64) {
            seeds64.resize((size_t)R * 16);
            omit64.resize(R);
            hkeys64.resize((size_t)R * 128);
            keep64.resize(R / 4);
            src64.resize((size_t)6 * R);
        }
    }
    SlotArrays arrays() {
        return {seeds.data(),   omit.data(),   hkeys.data(),   hco.data(),    hco64.data(), keep.data(), onm.data(), src.data(),
                seeds64.data(), omit64.data(), hkeys64.data(), keep64.data(), src64.data()};
    }
};
// The slot arrays of the groups groups[0 .. n_groups) (R = 8 * n_groups slots; group k's slot i is slot 8 * groups[k] + i of the
// proof) from a proof that passed check_records for them: omit / omit64 start at 8 (not opened), keep / keep64 at all ones,
// everything else at zero.  base[2k] / base[2k + 1] is added to group k's GF(2) / Z64 src / src64 offsets (the place of its
// records' bytes in the device buffer the unpack kernels read, minus their place in the proof; modulo 2^64).  The Z64 seeds,
// keys, omit64, keep64 and src64 are written only when has64 is set.
void fill_slots(const Parsed& P, const uint8_t* proof, const uint8_t* groups, uint32_t n_groups, const uint64_t* base, bool has64,
                const SlotArrays& a) {
    const uint32_t R = 8 * n_groups;
    const uint32_t NQ = R / 4;
    memset(a.seeds, 0, (size_t)R * 16);
    memset(a.omit, 8, R);
    memset(a.hkeys, 0, (size_t)R * 128);
    memset(a.hco, 0, (size_t)R * 32);
    memset(a.hco64, 0, (size_t)R * 32);
    std::fill_n(a.keep, NQ, 0xFFFFFFFFu);
    std::fill_n(a.onm, NQ, 0u);
    std::fill_n(a.src, (size_t)6 * R, (uint64_t)0);
    if (has64) {
        memset(a.seeds64, 0, (size_t)R * 16);
        memset(a.omit64, 8, R);
        memset(a.hkeys64, 0, (size_t)R * 128);
        std::fill_n(a.keep64, NQ, 0xFFFFFFFFu);
        std::fill_n(a.src64, (size_t)6 * R, (uint64_t)0);
    }
    for (uint32_t k = 0; k < n_groups; k++) {
        const uint32_t g0 = 8 * k, slot0 = 8u * groups[k];
        const uint64_t b2 = base[2 * k], b64 = base[2 * k + 1];
        if (slot0 < RV_ONLINE_REPS) {
            const OnRec* o = &P.gf2.on[slot0];
            const OnRec* z = &P.z64.on[slot0];
            for (int i = 0; i < 8; i++) {
                const uint32_t r = g0 + i;
                a.omit[r] = o[i].omit;
                a.src[0 * R + r] = b2 + o[i].rec;
                a.src[1 * R + r] = o[0].n_rec;
                a.src[2 * R + r] = b2 + o[i].corr;
                a.src[3 * R + r] = o[0].n_corr;
                a.src[4 * R + r] = b2 + o[i].in;
                a.src[5 * R + r] = o[0].n_in;
                a.keep[r / 4] &= ~(1u << (31 - 8 * (r % 4) - o[i].omit));  // BatchGen skips the omitted player
                a.onm[r / 4] |= 0xFFu << (24 - 8 * (r % 4));
                memcpy(a.hkeys + (size_t)r * 128, proof + o[i].keys, 128);  // the opened players' keys (online.rs:101-113)
                if (has64) {
                    // Z64 vectors: length of the group's first record, missing chunks read as zero
                    // (z64/recon.rs:68-108, z64/share.rs:51-91)
                    a.omit64[r] = z[i].omit;
                    a.keep64[r / 4] &= ~(1u << (31 - 8 * (r % 4) - z[i].omit));
                    a.src64[0 * R + r] = b64 + z[i].rec;
                    a.src64[1 * R + r] = std::min(z[i].n_rec, z[0].n_rec / 8 * 8);
                    a.src64[2 * R + r] = b64 + z[i].corr;
                    a.src64[3 * R + r] = std::min(z[i].n_corr, z[0].n_corr / 8 * 8);
                    a.src64[4 * R + r] = b64 + z[i].in;
                    a.src64[5 * R + r] = std::min(z[i].n_in, z[0].n_in / 8 * 8);
                    memcpy(a.hkeys64 + (size_t)r * 128, proof + z[i].keys, 128);
                }
            }
        } else {
            // seeds, and the online commitments the preprocessing slots carry over from the proof (preprocess.rs:55-57)
            const PreRec* q = &P.gf2.pre[slot0 - RV_ONLINE_REPS];
            const PreRec* q64 = &P.z64.pre[slot0 - RV_ONLINE_REPS];
            for (int i = 0; i < 8; i++) {
                const uint32_t r = g0 + i;
                memcpy(a.seeds + (size_t)r * 16, proof + q[i].seed, 16);
                memcpy(a.hco + (size_t)r * 32, proof + q[i].comm_online, 32);
                memcpy(a.hco64 + (size_t)r * 32, proof + q64[i].comm_online, 32);
                if (has64) memcpy(a.seeds64 + (size_t)r * 16, proof + q64[i].seed, 16);
            }
        }
    }
}
// ... of the slot range [slot_begin, slot_begin + R), every offset moved by `base` (the proof's place in the device buffer)
void fill_slots_range(const Parsed& P, const uint8_t* proof, uint32_t slot_begin, uint32_t R, uint64_t base, bool has64, const SlotArrays& a) {
    const std::vector<uint8_t> g = range_groups(slot_begin, R);
    const std::vector<uint64_t> b(2 * g.size(), base);
    fill_slots(P, proof, g.data(), (uint32_t)g.size(), b.data(), has64, a);
}
// the quad words that hold an opened repetition, in order, into quads[NQ]: their number
uint32_t opened_quads(const uint32_t* onm, uint32_t NQ, uint32_t* quads) {
    uint32_t n = 0;
    for (uint32_t q = 0; q < NQ; q++)
        if (onm[q]) quads[n++] = q;
    return n;
}
// rows of the GF(2) supplied values: sixteen quad words (two sectors, written whole) when the opened repetitions sit in the first
// sixteen -- the verifier's slot order puts them into the first ten -- instead of full share rows
uint32_t supplied_nq(const uint32_t* onm, uint32_t NQ) {
    for (uint32_t q = 16; q < NQ; q++)
        if (onm[q]) return NQ;
    return std::min(NQ, 16u);
}
// ... and the Z64 ones: the first 64 repetitions when no other is opened
uint32_t supplied_r64(const uint8_t* omit64, uint32_t R) {
    for (uint32_t r = 64; r < R; r++)
        if (omit64[r] < 8) return R;
    return std::min(R, 64u);
}
// the supplied-value rows of R slots, unpacked from the proof bytes at d_blob through the src / src64 table fill_slots wrote
void launch_unpack_supplied(hipStream_t st, const Compiled& cc, const uint8_t* d_blob, const uint64_t* d_src, const uint8_t* d_omit, uint32_t R,
                            uint32_t* d_in, uint32_t* d_corr, uint32_t* d_rec, uint32_t sup_nq) {
    launch_unpack_bits(st, d_blob, d_src + 4 * R, d_src + 5 * R, d_omit, cc.n_in, R / 4, 1, d_in, sup_nq);
    launch_unpack_bits(st, d_blob, d_src + 2 * R, d_src + 3 * R, d_omit, cc.n_pre, R / 4, 1, d_corr, sup_nq);
    launch_unpack_bits(st, d_blob, d_src + 0 * R, d_src + 1 * R, d_omit, cc.n_rec, R / 4, 0, d_rec, sup_nq);
}
void launch_unpack_supplied64(hipStream_t st, const Compiled& cc, const uint8_t* d_blob, const uint64_t* d_src64, const uint8_t* d_omit64, uint32_t R,
                              uint64_t* d_in, uint64_t* d_corr, uint64_t* d_rec, uint32_t sup_r) {
    launch_unpack64(st, d_blob, d_src64 + 4 * R, d_src64 + 5 * R, d_omit64, cc.n_in64, R, d_in, sup_r);
    launch_unpack64(st, d_blob, d_src64 + 2 * R, d_src64 + 3 * R, d_omit64, cc.n_corr64, R, d_corr, sup_r);
    launch_unpack64(st, d_blob, d_src64 + 0 * R, d_src64 + 1 * R, d_omit64, cc.n_rec64, R, d_rec, sup_r);
}
}  // namespace

// proof bytes the shard verifiers copied to the device (rv_hook_verify_proof_bytes)
static std::atomic<uint64_t> g_verify_proof_bytes{0};
extern "C" uint64_t rv_hook_verify_proof_bytes(void) { return g_verify_proof_bytes.load(std::memory_order_relaxed); }

// What one call of the single-proof verifier decides about its own order of work (DESIGN §12.1.1), from the circuit, the shape of
// the slots and where the proof's bytes are.  The environment is read at every call: tests switch it.
struct VerifySchedule {
    bool blob;         // every host array and the proof's runs in ONE copy through the page-locked input staging buffer
    bool side_copy;    // the proof's copy on the second stream, beside the mask kernels
    bool side_unpack;  // ... and the GF(2) unpack kernels there too
    bool split64;      // the fused Z64 verifier's quad groups without an opened repetition first, copy and unpack beside them
    bool z64f;         // k_z64_fused<VERIFY> (RV_Z64_FUSED_VERIFY=0: k_aes_z64_masks, then k_interp64 per level)
    bool overlap;      // the tail of the GF(2) masks beside the level launches (RV_OVERLAP, shard.inc)
    uint64_t ov_head;  // ... after the blocks the stand-alone generator writes first
    int vmode;         // MODE_VERIFY, or MODE_VERIFY_C (one u64 of corrections per row: internal.h)
};
// cumulative: calls, blob, side-stream copy, split64, fused Z64, overlap, MODE_VERIFY_C, calls on device memory
static std::atomic<uint64_t> g_verify_schedule[8];
extern "C" int rv_hook_verify_schedule(uint64_t out[8]) {
    if (!out) return RV_E_ARG;
    for (int i = 0; i < 8; i++) out[i] = g_verify_schedule[i].load(std::memory_order_relaxed);
    return RV_OK;
}
// blob_bytes: the host arrays and the proof's runs, packed; up_total: the runs alone.  device_src: the bytes lie in device memory
// (nothing to stage; the slot order makes NQ 64, sup_nq 16, sup_r 64 and opens ten quad words).
static VerifySchedule verify_schedule(rv_ctx* ctx, const rv_circuit* c, uint32_t NQ, bool has64, uint32_t sup_nq, uint32_t sup_r, uint32_t n_on_quads,
                                      size_t blob_bytes, size_t up_total, bool device_src) {
    const Compiled& cc = c->cc;
    VerifySchedule v{};
    // A small GF(2) proof goes over in ONE copy: every host array and the proof's runs are packed into the page-locked input
    // staging buffer and land in one device block (ten pageable copies of ~10 us each otherwise).  The call waits for the stream
    // before it returns, so the buffer is free again by the next call.
    v.blob = !device_src && !has64 && !g_recorder && blob_bytes <= rv_ctx::IN_STAGE_BYTES;
    if (v.blob && !ctx->h_in && hipHostMalloc((void**)&ctx->h_in, rv_ctx::IN_STAGE_BYTES, hipHostMallocDefault) != hipSuccess) {
        (void)hipGetLastError();
        ctx->h_in = nullptr;
        v.blob = false;
    }
    // One stream would queue the proof's copy up behind the mask kernels; from the second stream it runs beside them (copy
    // engine next to compute) and the unpack kernels wait for its event.  So do the GF(2) supplied-value rows (round 4): three
    // memory-bound transposes that find room beside the VALU-bound mask generator instead of standing between it and the
    // interpreter -- in device memory they go there behind the fill kernel.
    v.side_copy = !device_src && !v.blob && !g_recorder && up_total >= ((size_t)4 << 20);
    v.side_unpack = device_src || v.side_copy;
    // The verifier's Z64 half through k_z64_fused<VERIFY> as well.  Its kernels take 40 ms instead of 53 on the 10^6-MUL circuit;
    // the 640 MB proof's 12 ms of PCIe and the unpack kernels, which used to hide beside the mask generator, hide beside the quad
    // groups that hold no opened repetition (split64): rv_verify 59.5 -> 52.5 ms.
    v.z64f = has64 && c->z64f_ok && z64_fused_on() && z64_fused_supports(NQ) && !g_recorder &&
             !(getenv("RV_Z64_FUSED_VERIFY") && atoi(getenv("RV_Z64_FUSED_VERIFY")) == 0);
    // The fused Z64 verifier of a pure Z64 circuit whose opened repetitions all sit in the first quad group (sup_r == 64): only
    // that quad group's workgroups read supplied values, so the other groups' levels are queued FIRST (shard_run_levels), then the
    // proof's copy and the unpack kernels go to the side stream and hide beside them (a copy from pageable memory blocks the host
    // until the bytes are staged: issued up front it kept the level launches from being queued), and the first group's levels
    // wait for ev_sup64.
    v.split64 = has64 && v.z64f && cc.gates.empty() && v.side_copy && sup_r == 64 && NQ >= 32 && NQ % 16 == 0;
    {
        // RV_VERIFY_HEAD = the percentage of the GF(2) masks the stand-alone generator writes first, while the proof is on its way
        // (100 = all of them, the round-4 schedule)
        const int head_pct = getenv("RV_VERIFY_HEAD") ? std::min(std::max(atoi(getenv("RV_VERIFY_HEAD")), 0), 100) : 65;  // (100 / 90 / 75 / 60 / 40 / 0: 4.97 / 5.00 / 4.90 / 4.86 / 4.88 / 5.08 ms for rv_verify on the 10^7-gate circuit)
        const uint64_t n_blocks = cc.n_masks_pad / 128;
        const uint64_t ov_min = getenv("RV_OVERLAP_MIN") ? strtoull(getenv("RV_OVERLAP_MIN"), nullptr, 0) : 8192;
        const int ov_mode = getenv("RV_OVERLAP") ? atoi(getenv("RV_OVERLAP")) : 1;
        v.overlap = head_pct < 100 && ov_mode != 0 && !g_recorder && !v.blob && aes_col4_supports(NQ) && n_blocks >= ov_min;
        v.ov_head = v.overlap ? n_blocks * (uint64_t)head_pct / 100 : 0;
    }
    // Whole proofs of eligible circuits (the conditions of the prover's MODE_PROVE_V, and every opened repetition in the first
    // sixteen quad words -- the verifier's slot order puts them into the first ten): MODE_VERIFY_C (RV_VERIFY_VC=0: corr rows).
    // Not for gate streams with multi-base levels -- the prover's lazy linear forms: their kernel variant runs at 4 - 5 wavefronts
    // per SIMD either way and measured 0.07 ms SLOWER with the compact corrections; one-base streams: -0.03 ... -0.08 ms.
    const bool vc_on = !(getenv("RV_VERIFY_VC") && atoi(getenv("RV_VERIFY_VC")) == 0);
    v.vmode = vc_on && c->vclr_ok && !c->general_levels && NQ == 64 && sup_nq == 16 && n_on_quads && !g_recorder ? MODE_VERIFY_C : MODE_VERIFY;
    const bool counted[8] = {true, v.blob, v.side_copy, v.split64, v.z64f, v.overlap, v.vmode == MODE_VERIFY_C, device_src};
    for (int i = 0; i < 8; i++)
        if (counted[i]) g_verify_schedule[i].fetch_add(1, std::memory_order_relaxed);
    return v;
}

static int verify_groups_impl(rv_ctx* ctx, const rv_circuit* c, const uint8_t* proof, size_t proof_len, const uint8_t* groups,
                              uint32_t n_groups, uint8_t* digests, int* zero_checks_ok);

// RV_OK, or RV_E_ARG for an empty list, a group >= 32 or one given twice
static int groups_ok(const uint8_t* groups, uint32_t n_groups) {
    if (!groups || n_groups == 0 || n_groups > RV_TOTAL_REPS / 8) return RV_E_ARG;
    uint32_t seen = 0;
    for (uint32_t k = 0; k < n_groups; k++) {
        if (groups[k] >= RV_TOTAL_REPS / 8 || (seen >> groups[k]) & 1u) return RV_E_ARG;
        seen |= 1u << groups[k];
    }
    return RV_OK;
}

extern "C" int rv_verify_shard_groups(rv_ctx* ctx, const rv_circuit* c, const uint8_t* proof, size_t proof_len, const uint8_t* groups,
                                      uint32_t n_groups, uint8_t* digests, int* zero_checks_ok) {
    return guarded([&] { return verify_groups_impl(ctx, c, proof, proof_len, groups, n_groups, digests, zero_checks_ok); });
}

extern "C" int rv_verify_shard_ex(rv_ctx* ctx, const rv_circuit* c, const uint8_t* proof, size_t proof_len, uint32_t slot_begin,
                                  uint32_t slot_count, uint8_t* digests, int* zero_checks_ok) {
    if (slot_count == 0 || slot_count % 8 || slot_begin % 8 || slot_begin + slot_count > RV_TOTAL_REPS) return RV_E_ARG;
    return guarded([&] {
        const std::vector<uint8_t> g = range_groups(slot_begin, slot_count);
        return verify_groups_impl(ctx, c, proof, proof_len, g.data(), (uint32_t)g.size(), digests, zero_checks_ok);
    });
}

extern "C" int rv_verify_shard(rv_ctx* ctx, const rv_circuit* c, const uint8_t* proof, size_t proof_len, uint32_t slot_begin,
                               uint32_t slot_count, uint8_t* digests) {
    return rv_verify_shard_ex(ctx, c, proof, proof_len, slot_begin, slot_count, digests, nullptr);
}

// one domain's key material of R slots: every seed expanded, then the opened slots' keys from the proof (the omitted player's
// zeroed, online.rs:101-113)
static void launch_verifier_keys(hipStream_t st, uint32_t R, const uint8_t* d_seeds, const uint8_t* d_hkeys, const uint8_t* d_omit, uint8_t* d_keys) {
    launch_expand_seeds(st, d_seeds, R, d_keys);
    launch_overlay_rows(st, (uint32_t*)d_keys, (const uint32_t*)d_hkeys, d_omit, R, 32, 1);
}
// preprocessing slots: the online commitment is the one carried by the proof (preprocess.rs:55-57)
static void launch_carried_commitments(hipStream_t st, const rv_shard* s, const uint8_t* d_hco, const uint8_t* d_hco64) {
    const size_t DW = (size_t)s->R * 8;
    launch_overlay_rows(st, s->d_dig + 1 * DW, (const uint32_t*)d_hco, s->d_omit, s->R, 8, 0);
    launch_overlay_rows(st, s->d_dig + 3 * DW, (const uint32_t*)d_hco64, s->d_omit, s->R, 8, 0);
}

// ------------------------------------------------------------------------------------
// VerifyRun: one proof on its way through the single-proof verifier, in steps (DESIGN §12.1.1).  run() calls, in order: the
// SOURCE, which leaves the slot arrays in device memory -- from proof bytes in host memory (HostBytes: rv_verify*,
// rv_verify_shard*, any group list) or from a walked proof in device memory (d_table: rv_verify_device, groups 0 .. 31) --, then
// keys -> masks -> supplied_values -> params -> levels -> digests_out, which are shared.  A step returns RV_OK or the call's
// error code; run() gives the shard back on every way out.
// ------------------------------------------------------------------------------------
struct VerifyRun {
    // The host source's own state.  The proof bytes the unpack kernels read: the records of the listed online groups, nothing else
    // (a preprocessing slot's seed and online commitment go over in the host arrays).  A group's eight records are one span per
    // domain; spans that follow each other in the proof are one run and one copy, and every run keeps its offset modulo 16 (the
    // kernels' aligned loads see what they saw in the whole proof).
    struct HostBytes {
        struct Run {
            size_t begin, end, dst;
        };
        const uint8_t* proof;
        std::vector<Run> runs;
        size_t up_bytes = 0, up_total = 0;
        HostSlots H;
        std::vector<uint32_t> on_quads;
        hipEvent_t ev_arena = nullptr, ev_inputs = nullptr, ev_inputs64 = nullptr;  // side copy: what the second stream waits for

        HostBytes(const Parsed& P, const uint8_t* proof_, const uint8_t* groups, uint32_t n_groups, bool has64)
            : proof(proof_), H(8 * n_groups, has64), on_quads(2 * n_groups) {
            // base: what fill_slots adds to a group's offsets to land in the packed runs
            std::vector<uint64_t> base((size_t)2 * n_groups, 0);
            std::vector<uint32_t> run_of((size_t)2 * n_groups, 0);
            for (int dom = 0; dom < 2; dom++)
                for (uint32_t k = 0; k < n_groups; k++) {
                    if (8u * groups[k] >= RV_ONLINE_REPS) continue;
                    const Span sp = group_span(dom ? P.z64 : P.gf2, groups[k]);
                    if (runs.empty() || runs.back().end != sp.begin) runs.push_back({sp.begin, sp.begin, 0});
                    runs.back().end = sp.end;
                    run_of[2 * k + dom] = (uint32_t)runs.size() - 1;
                }
            for (Run& u : runs) {
                u.dst = ((up_total + 15) & ~(size_t)15) + u.begin % 16;
                up_total = u.dst + (u.end - u.begin);
                up_bytes += u.end - u.begin;
            }
            for (uint32_t k = 0; k < n_groups; k++)
                if (8u * groups[k] < RV_ONLINE_REPS)
                    for (int dom = 0; dom < 2; dom++) base[2 * k + dom] = (uint64_t)runs[run_of[2 * k + dom]].dst - (uint64_t)runs[run_of[2 * k + dom]].begin;
            fill_slots(P, proof, groups, n_groups, base.data(), has64, H.arrays());
            on_quads.resize(opened_quads(H.onm.data(), 2 * n_groups, on_quads.data()));
        }
    };

    rv_ctx* const ctx;
    const rv_circuit* const c;
    const Compiled& cc;
    const uint32_t R, NQ, rep_begin;
    const bool has64;
    HostBytes* const host;            // the source: host bytes ...
    const uint8_t* const d_bytes;     // ... or the first byte walked in device memory
    const uint64_t* const d_table;    //     and the walk's table
    rv_shard* s = nullptr;
    DevSlotArrays a{};                // the slot arrays in device memory (seeds, omit, omit64: the shard's own blocks)
    const uint8_t* d_base = nullptr;  // what the src / src64 offsets count from
    std::vector<uint32_t> on_quads;   // the device source's (the slot order's)
    uint32_t n_on_quads = 0, sup_nq = 0, sup_r = 0;
    uint32_t *d_sup_in = nullptr, *d_sup_corr = nullptr, *d_sup_rec = nullptr;
    uint64_t *d_sup_in64 = nullptr, *d_sup_corr64 = nullptr, *d_sup_rec64 = nullptr;
    VerifySchedule sch{};
    hipEvent_t ev_unpacked = nullptr;  // device source: the GF(2) supplied values are unpacked on the second stream
    InterpParams p{};
    Interp64Params p64{};

    VerifyRun(rv_ctx* ctx_, const rv_circuit* c_, uint32_t R_, uint32_t rep_begin_, HostBytes* host_, const uint8_t* d_bytes_, const uint64_t* d_table_)
        : ctx(ctx_), c(c_), cc(c_->cc), R(R_), NQ(R_ / 4), rep_begin(rep_begin_), has64(!c_->cc.gates64.empty()), host(host_), d_bytes(d_bytes_),
          d_table(d_table_) {}

    int run(uint8_t* digests, int* zero_checks_ok) {
        s = new rv_shard();
        s->ctx = ctx;
        s->c = c;
        s->rep_begin = rep_begin;  // (read by the prover's openings only)
        s->R = R;
        s->NQ = NQ;
        const int rc = issue(digests, zero_checks_ok);
        rv_shard_destroy(s);
        return rc;
    }

    int issue(uint8_t* digests, int* zero_checks_ok) {
        int rc;
        if ((rc = host ? source_host() : source_device()) || (rc = keys()) || (rc = masks()) || (rc = supplied_values()) || (rc = params()) ||
            (rc = levels()))
            return rc;
        return digests_out(digests, zero_checks_ok);
    }

    // a device block the shard gives back with its `extra` list
    template <class T>
    int tracked(size_t count, T*& ptr) {
        const int rc = dalloc(ctx, count, &ptr);
        if (!rc) s->extra.push_back(ptr);
        return rc;
    }
    hipEvent_t event() {
        hipEvent_t e = ctx->get_sync_event();
        s->misc_events.push_back(e);
        return e;
    }
    // the supplied-value rows of both sources, and the Z64 side's arrays
    int alloc_rest() {
        int rc;
        if ((rc = tracked((size_t)std::max<uint64_t>(cc.n_in, 1) * sup_nq, d_sup_in)) || (rc = tracked((size_t)std::max<uint64_t>(cc.n_pre, 1) * sup_nq, d_sup_corr)) ||
            (rc = tracked((size_t)std::max<uint64_t>(cc.n_rec, 1) * sup_nq, d_sup_rec)))
            return rc;
        if (!has64) return RV_OK;
        if ((rc = dalloc(ctx, (size_t)R * 128, &s->d_keys64)) || (rc = dalloc(ctx, R, &s->d_omit64))) return rc;
        a.omit64 = s->d_omit64;
        if ((rc = tracked((size_t)R * 16, a.seeds64)) || (rc = tracked((size_t)R * 128, a.hkeys64)) || (rc = tracked(NQ, a.keep64)) ||
            (rc = tracked((size_t)6 * R, a.src64)) || (rc = tracked((size_t)std::max<uint64_t>(cc.n_in64, 1) * sup_r, d_sup_in64)) ||
            (rc = tracked((size_t)std::max<uint64_t>(cc.n_corr64, 1) * sup_r, d_sup_corr64)) ||
            (rc = tracked((size_t)std::max<uint64_t>(cc.n_rec64, 1) * sup_r, d_sup_rec64)))
            return rc;
        return RV_OK;
    }

    // ---- source, host bytes: the schedule, then the arrays over in one blob or in separate copies.  The proof itself follows in
    //      supplied_values (side copy: on the second stream, behind ev_arena and ev_inputs; split64: from inside the level loop)
    int source_host() {
        HostBytes& h = *host;
        HostSlots& H = h.H;
        n_on_quads = (uint32_t)h.on_quads.size();
        sup_nq = supplied_nq(H.onm.data(), NQ);
        sup_r = has64 ? supplied_r64(H.omit64.data(), R) : R;
        size_t blob_bytes = 0;
        auto seg = [&](size_t len) {
            const size_t o = blob_bytes;
            blob_bytes += (len + 15) & ~(size_t)15;
            return o;
        };
        const size_t o_seeds = seg(H.seeds.size()), o_omit = seg(H.omit.size()), o_keep = seg((size_t)NQ * 4), o_onm = seg((size_t)NQ * 4),
                     o_onq = seg(std::max<size_t>(h.on_quads.size(), 1) * 4), o_hkeys = seg(H.hkeys.size()), o_hco = seg(H.hco.size()),
                     o_hco64 = seg(H.hco64.size()), o_src = seg(H.src.size() * 8), o_proof = seg(h.up_total);
        sch = verify_schedule(ctx, c, NQ, has64, sup_nq, sup_r, n_on_quads, blob_bytes, h.up_total, false);
        int rc;
        uint8_t* d_proof = nullptr;
        uint32_t* d_on_quads = nullptr;
        if (sch.blob) {
            if ((rc = dalloc(ctx, blob_bytes, &s->d_seeds)) || (rc = dalloc(ctx, (size_t)R * 128, &s->d_keys))) return rc;
            uint8_t* b = s->d_seeds;  // (pointers inside d_seeds' block: the arena ignores them on release)
            s->d_omit = b + o_omit;
            a.keep = (uint32_t*)(b + o_keep);
            a.onm = (uint32_t*)(b + o_onm);
            d_on_quads = (uint32_t*)(b + o_onq);
            a.hkeys = b + o_hkeys;
            a.hco = b + o_hco;
            a.hco64 = b + o_hco64;
            a.src = (uint64_t*)(b + o_src);
            d_proof = b + o_proof;
            uint8_t* hb = ctx->h_in;
            memcpy(hb + o_seeds, H.seeds.data(), H.seeds.size());
            memcpy(hb + o_omit, H.omit.data(), H.omit.size());
            memcpy(hb + o_keep, H.keep.data(), (size_t)NQ * 4);
            memcpy(hb + o_onm, H.onm.data(), (size_t)NQ * 4);
            if (!h.on_quads.empty()) memcpy(hb + o_onq, h.on_quads.data(), h.on_quads.size() * 4);
            memcpy(hb + o_hkeys, H.hkeys.data(), H.hkeys.size());
            memcpy(hb + o_hco, H.hco.data(), H.hco.size());
            memcpy(hb + o_hco64, H.hco64.data(), H.hco64.size());
            memcpy(hb + o_src, H.src.data(), H.src.size() * 8);
            for (const auto& u : h.runs) memcpy(hb + o_proof + u.dst, h.proof + u.begin, u.end - u.begin);
        } else {
            if ((rc = dalloc(ctx, (size_t)R * 16, &s->d_seeds)) || (rc = dalloc(ctx, (size_t)R * 128, &s->d_keys)) || (rc = dalloc(ctx, R, &s->d_omit)) ||
                (rc = tracked(std::max<size_t>(h.up_total, 1), d_proof)) || (rc = tracked(H.src.size(), a.src)))
                return rc;
            // d_proof / a.src may be filled from the SECOND stream further down (beside the mask kernels).  The arena hands blocks out
            // in the main stream's order, so the side stream first waits for everything the main stream holds NOW -- whatever used
            // these blocks last -- and nothing of this call's own kernels (they are queued after this point)
            if (sch.side_copy) {
                h.ev_arena = event();
                HIPCHK(hipEventRecord(h.ev_arena, ctx->stream));
            }
            if ((rc = tracked(NQ, a.keep)) || (rc = tracked(NQ, a.onm)) || (rc = tracked(std::max<size_t>(h.on_quads.size(), 1), d_on_quads)) ||
                (rc = tracked(H.hkeys.size(), a.hkeys)) || (rc = tracked(H.hco.size(), a.hco)) || (rc = tracked(H.hco64.size(), a.hco64)))
                return rc;
        }
        a.seeds = s->d_seeds;
        a.omit = s->d_omit;
        d_base = d_proof;
        if ((rc = alloc_rest())) return rc;
        // ---- stream 1: everything the mask generator needs
        if (sch.blob) {
            HIPCHK(hipMemcpyAsync(s->d_seeds, ctx->h_in, blob_bytes, hipMemcpyHostToDevice, ctx->stream));
        } else {
            HIPCHK(hipMemcpyAsync(s->d_seeds, H.seeds.data(), H.seeds.size(), hipMemcpyHostToDevice, ctx->stream));
            HIPCHK(hipMemcpyAsync(s->d_omit, H.omit.data(), H.omit.size(), hipMemcpyHostToDevice, ctx->stream));
            HIPCHK(hipMemcpyAsync(a.keep, H.keep.data(), NQ * 4, hipMemcpyHostToDevice, ctx->stream));
            HIPCHK(hipMemcpyAsync(a.onm, H.onm.data(), NQ * 4, hipMemcpyHostToDevice, ctx->stream));
            if (!h.on_quads.empty()) HIPCHK(hipMemcpyAsync(d_on_quads, h.on_quads.data(), h.on_quads.size() * 4, hipMemcpyHostToDevice, ctx->stream));
            HIPCHK(hipMemcpyAsync(a.hkeys, H.hkeys.data(), H.hkeys.size(), hipMemcpyHostToDevice, ctx->stream));
            HIPCHK(hipMemcpyAsync(a.hco, H.hco.data(), H.hco.size(), hipMemcpyHostToDevice, ctx->stream));
            HIPCHK(hipMemcpyAsync(a.hco64, H.hco64.data(), H.hco64.size(), hipMemcpyHostToDevice, ctx->stream));
        }
        s->d_on_quads = d_on_quads;
        s->n_on_quads = n_on_quads;
        if (sch.side_copy) {  // (the side stream's unpack kernels read d_omit: uploaded by now)
            h.ev_inputs = event();
            HIPCHK(hipEventRecord(h.ev_inputs, ctx->stream));
        }
        if (has64) {
            HIPCHK(hipMemcpyAsync(a.seeds64, H.seeds64.data(), H.seeds64.size(), hipMemcpyHostToDevice, ctx->stream));
            HIPCHK(hipMemcpyAsync(s->d_omit64, H.omit64.data(), H.omit64.size(), hipMemcpyHostToDevice, ctx->stream));
            HIPCHK(hipMemcpyAsync(a.keep64, H.keep64.data(), NQ * 4, hipMemcpyHostToDevice, ctx->stream));
            HIPCHK(hipMemcpyAsync(a.hkeys64, H.hkeys64.data(), H.hkeys64.size(), hipMemcpyHostToDevice, ctx->stream));
        }
        return RV_OK;
    }

    // ---- source, device bytes (a walk that ended VW_OK): k_fill_slots_dev writes the arrays; the unpack kernels read the caller's
    //      buffer in place, the GF(2) ones on the second stream behind the fill kernel and whatever used their blocks last
    int source_device() {
        on_quads.resize(RV_ONLINE_REPS / 4);  // what follows from the slot order alone (online records first)
        for (uint32_t q = 0; q < on_quads.size(); q++) on_quads[q] = q;
        n_on_quads = (uint32_t)on_quads.size();
        sup_nq = std::min(NQ, 16u);
        sup_r = has64 ? 64u : R;
        sch = verify_schedule(ctx, c, NQ, has64, sup_nq, sup_r, n_on_quads, 0, 0, true);
        int rc;
        uint32_t* d_on_quads = nullptr;
        if ((rc = dalloc(ctx, (size_t)R * 16, &s->d_seeds)) || (rc = dalloc(ctx, (size_t)R * 128, &s->d_keys)) || (rc = dalloc(ctx, R, &s->d_omit))) return rc;
        a.seeds = s->d_seeds;
        a.omit = s->d_omit;
        d_base = d_bytes;
        if ((rc = tracked((size_t)R * 128, a.hkeys)) || (rc = tracked((size_t)R * 32, a.hco)) || (rc = tracked((size_t)R * 32, a.hco64)) ||
            (rc = tracked(NQ, a.keep)) || (rc = tracked(NQ, a.onm)) || (rc = tracked((size_t)6 * R, a.src)) || (rc = tracked(on_quads.size(), d_on_quads)) ||
            (rc = alloc_rest()))
            return rc;
        launch_fill_slots_dev(ctx->stream, d_bytes, d_table, has64, a);
        HIPCHK(hipGetLastError());
        HIPCHK(hipMemcpyAsync(d_on_quads, on_quads.data(), on_quads.size() * 4, hipMemcpyHostToDevice, ctx->stream));
        s->d_on_quads = d_on_quads;
        s->n_on_quads = n_on_quads;
        hipEvent_t ev_filled = event();
        ev_unpacked = event();
        HIPCHK(hipEventRecord(ev_filled, ctx->stream));
        HIPCHK(hipStreamWaitEvent(ctx->stream2, ev_filled, 0));
        launch_unpack_supplied(ctx->stream2, cc, d_base, a.src, s->d_omit, R, d_sup_in, d_sup_corr, d_sup_rec, sup_nq);
        HIPCHK(hipEventRecord(ev_unpacked, ctx->stream2));
        return RV_OK;
    }

    int keys() {
        ctx->phase(RV_PH_SETUP);
        ctx->count(2);
        launch_verifier_keys(ctx->stream, R, s->d_seeds, a.hkeys, s->d_omit, s->d_keys);
        if (has64) {
            launch_verifier_keys(ctx->stream, R, a.seeds64, a.hkeys64, s->d_omit64, s->d_keys64);
            ctx->count(2);
        }
        ctx->phase(-1);
        if (host && host->ev_arena && has64) {
            host->ev_inputs64 = event();
            HIPCHK(hipEventRecord(host->ev_inputs64, ctx->stream));
        }
        return RV_OK;
    }

    // the schedule's switches into the shard; key schedule, bitslice, the mask generators (shard.inc)
    int masks() {
        s->z64f = sch.z64f;
        s->overlap = sch.overlap;
        s->ov_head = sch.ov_head;
        return shard_setup_prg(s, a.keep, a.keep64);
    }

    // ---- the supplied-value rows, unpacked from the proof bytes at d_base through the src / src64 tables
    int supplied_values() {
        hipStream_t sb = ctx->stream;
        if (!host) {
            HIPCHK(hipStreamWaitEvent(sb, ev_unpacked, 0));
        } else {
            // the interpreter's stream: the proof itself (tens of MB from pageable memory: the host blocks in this copy while the mask
            // kernels above already run) and the GF(2) rows unpacked from it -- or the second stream for both (side copy)
            HostBytes& h = *host;
            uint8_t* d_proof = const_cast<uint8_t*>(d_base);
            hipStream_t su = sb;  // the stream of the GF(2) unpack kernels
            if (!sch.blob && !sch.split64) {
                hipStream_t sc = sch.side_copy ? ctx->stream2 : sb;
                if (sc != sb) HIPCHK(hipStreamWaitEvent(sc, h.ev_arena, 0));
                for (const auto& u : h.runs) HIPCHK(hipMemcpyAsync(d_proof + u.dst, h.proof + u.begin, u.end - u.begin, hipMemcpyHostToDevice, sc));
                HIPCHK(hipMemcpyAsync(a.src, h.H.src.data(), h.H.src.size() * 8, hipMemcpyHostToDevice, sc));
                if (sc != sb) {
                    HIPCHK(hipStreamWaitEvent(sc, h.ev_inputs, 0));
                    su = sc;
                }
            }
            if (!sch.split64) {  // (split64: a circuit without GF(2) gates has none of these)
                launch_unpack_supplied(su, cc, d_proof, a.src, s->d_omit, R, d_sup_in, d_sup_corr, d_sup_rec, sup_nq);
                if (su != sb) {
                    hipEvent_t e = event();
                    HIPCHK(hipEventRecord(e, su));
                    HIPCHK(hipStreamWaitEvent(sb, e, 0));
                }
            }
            if (sch.split64) {
                s->ev_sup64 = event();
                s->mid64 = [this, &h, d_proof]() -> int {
                    hipStream_t sc = ctx->stream2;
                    bool copied = hipStreamWaitEvent(sc, h.ev_arena, 0) == hipSuccess;
                    for (const auto& u : h.runs)
                        copied = copied && hipMemcpyAsync(d_proof + u.dst, h.proof + u.begin, u.end - u.begin, hipMemcpyHostToDevice, sc) == hipSuccess;
                    if (!copied || hipStreamWaitEvent(sc, h.ev_inputs64, 0) != hipSuccess ||
                        hipMemcpyAsync(a.src64, h.H.src64.data(), h.H.src64.size() * 8, hipMemcpyHostToDevice, sc) != hipSuccess)
                        return hip_fail(hipGetLastError(), "rv_verify: the proof's copy", __FILE__, __LINE__);
                    launch_unpack_supplied64(sc, cc, d_proof, a.src64, s->d_omit64, R, d_sup_in64, d_sup_corr64, d_sup_rec64, sup_r);
                    if (hipEventRecord(s->ev_sup64, sc) != hipSuccess) return hip_fail(hipGetLastError(), "hipEventRecord", __FILE__, __LINE__);
                    return RV_OK;
                };
            } else if (has64) {
                HIPCHK(hipMemcpyAsync(a.src64, h.H.src64.data(), h.H.src64.size() * 8, hipMemcpyHostToDevice, sb));
            }
        }
        if (has64 && !sch.split64) launch_unpack_supplied64(sb, cc, d_base, a.src64, s->d_omit64, R, d_sup_in64, d_sup_corr64, d_sup_rec64, sup_r);
        return RV_OK;
    }

    int params() {
        if (has64) {
            p64.omit = s->d_omit64;
            p64.sup_in = d_sup_in64;
            p64.sup_corr = d_sup_corr64;
            p64.sup_rec = d_sup_rec64;
            p64.sup_r = sup_r;
        }
        p.on_mask = a.onm;
        p.sup_in = d_sup_in;
        p.sup_corr = d_sup_corr;
        p.sup_rec = d_sup_rec;
        p.sup_nq = sup_nq;
        if (sch.vmode == MODE_VERIFY_C) {
            uint64_t* d_vc = nullptr;
            if (int rc = tracked((size_t)cc.n_rows, d_vc)) return rc;
            HIPCHK(hipMemsetAsync(d_vc + cc.zero_row, 0, 8, ctx->stream));
            p.vc = d_vc;
            g_verify_vc.fetch_add(1, std::memory_order_relaxed);
        }
        return RV_OK;
    }

    int levels() {
        if (int rc = shard_run(s, sch.vmode, p, p64)) return rc;
        launch_carried_commitments(ctx->stream, s, a.hco, a.hco64);
        return shard_join(s);
    }

    // The digests and the flag word leave through the mapped staging buffer (one small kernel instead of two copy-engine
    // operations of ~25 us each; see rv_prove_impl), unless it could not be had.  zero_checks_ok may be null.
    int digests_out(uint8_t* digests, int* zero_checks_ok) {
        int dev_flags = 0;  // RV_DEV_ZERO_CHECK: an AssertZero of an opened repetition did not reconstruct to zero
        uint8_t* const stage_dev = g_recorder ? nullptr : ctx->stage_mapped();
        if (stage_dev) {
            launch_store_words(ctx->stream, (const uint32_t*)s->d_h, R * 8, (uint32_t*)stage_dev, zero_checks_ok ? s->d_err : nullptr, (int*)(stage_dev + (size_t)R * 32));
            HIPCHK(hipStreamSynchronize(ctx->stream));
            memcpy(digests, ctx->h_stage, (size_t)R * 32);
            if (zero_checks_ok) memcpy(&dev_flags, ctx->h_stage + (size_t)R * 32, sizeof dev_flags);
        } else {
            HIPCHK(hipMemcpyAsync(digests, s->d_h, (size_t)R * 32, hipMemcpyDeviceToHost, ctx->stream));
            if (zero_checks_ok) HIPCHK(hipMemcpyAsync(&dev_flags, s->d_err, sizeof dev_flags, hipMemcpyDeviceToHost, ctx->stream));
            HIPCHK(hipStreamSynchronize(ctx->stream));
        }
        if (zero_checks_ok) *zero_checks_ok = !(dev_flags & RV_DEV_ZERO_CHECK);
        if (host) g_verify_proof_bytes.fetch_add(host->up_bytes, std::memory_order_relaxed);
        ctx->collect();
        ctx->prof.calls++;
        return RV_OK;
    }
};

static int verify_groups_impl(rv_ctx* ctx, const rv_circuit* c, const uint8_t* proof, size_t proof_len, const uint8_t* groups,
                              uint32_t n_groups, uint8_t* digests, int* zero_checks_ok) {
    LibBusy busy_guard;  // (compile.h: the background unmapper keeps still while the GPU is driven)
    if (!ctx || !c || !proof || !digests || groups_ok(groups, n_groups)) return RV_E_ARG;
    Parsed P;
    int rc = parse_proof(proof, proof_len, P);
    if (rc) return rc;
    if (!format_ok(P)) return RV_E_PROOF_MALFORMED;  // callers check the format first (rv_verify returns ok=0)
    HIPCHK(hipSetDevice(ctx->device));
    if (int rs2 = ctx_stream2(ctx)) return rs2;
    if ((rc = check_records(P, groups, n_groups))) return rc;
    VerifyRun::HostBytes bytes(P, proof, groups, n_groups, !c->cc.gates64.empty());
    return VerifyRun(ctx, c, 8 * n_groups, 8u * groups[0], &bytes, nullptr, nullptr).run(digests, zero_checks_ok);
}

// Verification is STRICT unless the caller asks for the reference's behaviour (RV_VERIFY_REFERENCE_COMPAT): flags 0 and
// RV_VERIFY_STRICT mean the same thing; both bits together are a contradiction
static bool verify_flags_ok(uint32_t flags) {
    return !(flags & ~(uint32_t)(RV_VERIFY_STRICT | RV_VERIFY_REFERENCE_COMPAT)) &&
           (flags & (RV_VERIFY_STRICT | RV_VERIFY_REFERENCE_COMPAT)) != (RV_VERIFY_STRICT | RV_VERIFY_REFERENCE_COMPAT);
}
static bool verify_is_strict(uint32_t flags) { return !(flags & RV_VERIFY_REFERENCE_COMPAT); }

// The two halves of the final decision, shared by the host-bytes form below and the device form (verify_dev.inc), which has comm
// and the records' omit bytes without a host copy of the proof.
// The reference's check: the challenge comm opens (omit[256]), and whether the slot digests, put back into repetition order, hash to comm
static bool digests_give_comm(const uint8_t comm[32], const uint8_t* slot_digests, uint8_t omit[RV_TOTAL_REPS]) {
    rv_challenge(comm, omit);  // proof/mod.rs:290
    b3::Hasher hs;
    size_t on = 0, pre = RV_ONLINE_REPS;
    for (int i = 0; i < RV_TOTAL_REPS; i++) hs.update(slot_digests + 32 * (omit[i] < 8 ? on++ : pre++), 32);
    uint8_t again[32];
    hs.finalize(again);
    return memcmp(again, comm, 32) == 0;
}
// ... and the strict one: the 40 online records of both domains name the player the challenge omits
static bool records_omit_challenge(const uint8_t omit[RV_TOTAL_REPS], const uint8_t* rec_omit2, const uint8_t* rec_omit64) {
    bool same = true;
    size_t k = 0;
    for (int i = 0; i < RV_TOTAL_REPS; i++)
        if (omit[i] < 8) {
            if (rec_omit2[k] != omit[i] || rec_omit64[k] != omit[i]) same = false;
            k++;
        }
    return same;
}

static int rv_verify_finish_impl(const uint8_t* proof, size_t proof_len, const uint8_t* slot_digests, uint32_t flags,
                                 int zero_checks_ok, int* ok) {
    if (!proof || !slot_digests || !ok || proof_len < 32 || !verify_flags_ok(flags)) return RV_E_ARG;
    uint8_t omit[RV_TOTAL_REPS];
    *ok = digests_give_comm(proof, slot_digests, omit);
    if (verify_is_strict(flags)) {
        // SURVEY F9: the reference computes `okay` without reading it (online.rs:21,175-177) and only checks WHICH
        // repetitions are opened, never the records' omitted player (proof/mod.rs:292-302)
        if (!zero_checks_ok) *ok = 0;
        Parsed P;
        int rc = parse_proof(proof, proof_len, P);
        if (rc) return rc;
        if (!format_ok(P)) {
            *ok = 0;
            return RV_OK;
        }
        uint8_t rec2[RV_ONLINE_REPS], rec64[RV_ONLINE_REPS];
        for (int k = 0; k < RV_ONLINE_REPS; k++) rec2[k] = P.gf2.on[k].omit, rec64[k] = P.z64.on[k].omit;
        if (!records_omit_challenge(omit, rec2, rec64)) *ok = 0;
    }
    return RV_OK;
}

extern "C" int rv_verify_finish_ex(const uint8_t* proof, size_t proof_len, const uint8_t* slot_digests, uint32_t flags,
                                   int zero_checks_ok, int* ok) {
    return guarded([&] { return rv_verify_finish_impl(proof, proof_len, slot_digests, flags, zero_checks_ok, ok); });
}

extern "C" int rv_verify_finish(const uint8_t* proof, size_t proof_len, const uint8_t* slot_digests, int* ok) {
    // no zero-check input here: this entry point is the reference's final check and nothing more (see the header)
    return rv_verify_finish_ex(proof, proof_len, slot_digests, RV_VERIFY_REFERENCE_COMPAT, 1, ok);
}

static int rv_verify_impl(rv_ctx* ctx, const rv_circuit* c, const uint8_t* proof, size_t proof_len, uint32_t flags, int* ok);

extern "C" int rv_verify_ex(rv_ctx* ctx, const rv_circuit* c, const uint8_t* proof, size_t proof_len, uint32_t flags, int* ok) {
    return guarded([&] { return rv_verify_impl(ctx, c, proof, proof_len, flags, ok); });
}

extern "C" int rv_verify(rv_ctx* ctx, const rv_circuit* c, const uint8_t* proof, size_t proof_len, int* ok) {
    return rv_verify_ex(ctx, c, proof, proof_len, 0, ok);  // flags 0 = strict
}

static int rv_verify_impl(rv_ctx* ctx, const rv_circuit* c, const uint8_t* proof, size_t proof_len, uint32_t flags, int* ok) {
    if (!ctx || !c || !proof || !ok || !verify_flags_ok(flags)) return RV_E_ARG;
    *ok = 0;
    Parsed P;
    int rc = parse_proof(proof, proof_len, P);
    if (rc) return rc;
    if (!format_ok(P)) return RV_OK;  // wrong repetition counts: `false`, not an error (proof/mod.rs:225-230)
    std::vector<uint8_t> dig(RV_TOTAL_REPS * 32);
    int zc = 1;
    if ((rc = rv_verify_shard_ex(ctx, c, proof, proof_len, 0, RV_TOTAL_REPS, dig.data(), &zc))) return rc;
    return rv_verify_finish_ex(proof, proof_len, dig.data(), flags, zc, ok);
}
