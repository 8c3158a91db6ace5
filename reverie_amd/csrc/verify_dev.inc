// Part of api.hip (#included there, one translation unit, behind verify.inc): rv_verify_device / rv_verify_sections_device --
// Proof::verify on proof bytes in device memory (verify_dev.h: the walk, the table, the two kernels).
//
// The call: k_parse_proof walks the framing, the host waits for its status word (with comm and the 80 omit bytes: 120 bytes through
// the mapped staging buffer).  A good status: k_fill_slots_dev writes the slot arrays and the verifier's pipeline runs as in
// verify_groups_impl, the unpack kernels reading the caller's buffer in place -- no proof byte crosses to the host.  Any other
// status: the bytes are copied to the host and rv_verify_ex answers, so the answer for bytes that are not a well-framed proof of
// acceptable records is the host verifier's by construction.
//
// Ordering: there is no upload to hide, so none of the host form's staging (blob, the side-stream copy, split64).  Everything runs
// on the context's stream except the three GF(2) unpack kernels, which go to the second stream behind the fill kernel and run
// beside the mask generator as they do in the host form; the levels wait for their event.

static std::atomic<uint64_t> g_verify_dev_paths[2];  // calls that took {the device path, the host fallback}
extern "C" int rv_hook_verify_device_paths(uint64_t out[2]) {
    if (!out) return RV_E_ARG;
    out[0] = g_verify_dev_paths[0].load(std::memory_order_relaxed);
    out[1] = g_verify_dev_paths[1].load(std::memory_order_relaxed);
    return RV_OK;
}

// RV_OK when p is an address aligned to `align` bytes (a power of two) in the memory of the context's device and, where the runtime
// can tell, p[0, len) lies inside its allocation; RV_E_ARG otherwise (host memory, another device's)
static int device_bytes_ok(rv_ctx* ctx, const void* p, size_t len, size_t align) {
    if ((uintptr_t)p & (align - 1)) return RV_E_ARG;
    hipPointerAttribute_t at;
    if (hipPointerGetAttributes(&at, p) != hipSuccess) {  // (plain host memory: an error with some runtimes, "unregistered" with others)
        (void)hipGetLastError();
        return RV_E_ARG;
    }
    if (at.type != hipMemoryTypeDevice || at.device != ctx->device) return RV_E_ARG;
    void* base = nullptr;
    size_t size = 0;
    if (hipMemGetAddressRange(&base, &size, const_cast<void*>(p)) != hipSuccess) {
        (void)hipGetLastError();  // (memory the runtime keeps no range for: the caller's word for len stands)
        return RV_OK;
    }
    const size_t before = (size_t)((const uint8_t*)p - (const uint8_t*)base);
    return (before <= size && len <= size - before) ? RV_OK : RV_E_ARG;
}

// The verifier's 256 slot digests and zero-check flag from a proof in device memory whose walk ended VW_OK: d_bytes is the first
// byte walked, d_table the walk's table.  verify_groups_impl for groups 0 .. 31 with the slot arrays made on the device.
static int verify_device_slots(rv_ctx* ctx, const rv_circuit* c, const uint8_t* d_bytes, const uint64_t* d_table, uint8_t* digests,
                               int* zero_checks_ok) {
    const Compiled& cc = c->cc;
    constexpr uint32_t R = RV_TOTAL_REPS, NQ = R / 4;
    const bool has64 = !cc.gates64.empty();
    // what follows from the slot order alone (online records first): the opened quad words, the supplied rows' widths
    std::vector<uint32_t> on_quads(RV_ONLINE_REPS / 4);
    for (uint32_t q = 0; q < on_quads.size(); q++) on_quads[q] = q;
    const uint32_t sup_nq = std::min(NQ, 16u), sup_r = has64 ? 64u : R;

    rv_shard* s = new rv_shard();
    s->ctx = ctx;
    s->c = c;
    s->rep_begin = 0;
    s->R = R;
    s->NQ = NQ;
    auto fail = [&](int code) {
        rv_shard_destroy(s);
        return code;
    };
    auto track = [&](void* p) { s->extra.push_back(p); };
    int rc;
#define DA(count, ptr)                                     \
    do {                                                   \
        if ((rc = dalloc(ctx, (count), &(ptr)))) return fail(rc); \
        track(ptr);                                        \
    } while (0)
#define HC(x)                                                    \
    do {                                                         \
        if ((x) != hipSuccess) {                                 \
            hip_fail(hipGetLastError(), #x, __FILE__, __LINE__); \
            return fail(RV_E_DEVICE);                            \
        }                                                        \
    } while (0)
    DevSlotArrays a{};
    uint32_t *d_on_quads = nullptr, *d_sup_in = nullptr, *d_sup_corr = nullptr, *d_sup_rec = nullptr;
    if ((rc = dalloc(ctx, (size_t)R * 16, &s->d_seeds)) || (rc = dalloc(ctx, (size_t)R * 128, &s->d_keys)) || (rc = dalloc(ctx, R, &s->d_omit)))
        return fail(rc);
    a.seeds = s->d_seeds;
    a.omit = s->d_omit;
    DA((size_t)R * 128, a.hkeys);
    DA((size_t)R * 32, a.hco);
    DA((size_t)R * 32, a.hco64);
    DA(NQ, a.keep);
    DA(NQ, a.onm);
    DA((size_t)6 * R, a.src);
    DA(on_quads.size(), d_on_quads);
    DA((size_t)std::max<uint64_t>(cc.n_in, 1) * sup_nq, d_sup_in);
    DA((size_t)std::max<uint64_t>(cc.n_pre, 1) * sup_nq, d_sup_corr);
    DA((size_t)std::max<uint64_t>(cc.n_rec, 1) * sup_nq, d_sup_rec);
    uint64_t *d_sup_in64 = nullptr, *d_sup_corr64 = nullptr, *d_sup_rec64 = nullptr;
    if (has64) {
        if ((rc = dalloc(ctx, (size_t)R * 128, &s->d_keys64)) || (rc = dalloc(ctx, R, &s->d_omit64))) return fail(rc);
        a.omit64 = s->d_omit64;
        DA((size_t)R * 16, a.seeds64);
        DA((size_t)R * 128, a.hkeys64);
        DA(NQ, a.keep64);
        DA((size_t)6 * R, a.src64);
        DA((size_t)std::max<uint64_t>(cc.n_in64, 1) * sup_r, d_sup_in64);
        DA((size_t)std::max<uint64_t>(cc.n_corr64, 1) * sup_r, d_sup_corr64);
        DA((size_t)std::max<uint64_t>(cc.n_rec64, 1) * sup_r, d_sup_rec64);
    }
    const size_t DW = (size_t)R * 8;
    // ---- the slot arrays, then everything the mask generator needs and the masks themselves
    launch_fill_slots_dev(ctx->stream, d_bytes, d_table, has64, a);
    HC(hipGetLastError());
    HC(hipMemcpyAsync(d_on_quads, on_quads.data(), on_quads.size() * 4, hipMemcpyHostToDevice, ctx->stream));
    s->d_on_quads = d_on_quads;
    s->n_on_quads = (uint32_t)on_quads.size();
    // the GF(2) supplied-value rows on the second stream, behind the fill kernel and whatever used their blocks last
    hipEvent_t ev_filled = ctx->get_sync_event(), ev_unpacked = ctx->get_sync_event();
    s->misc_events.push_back(ev_filled);
    s->misc_events.push_back(ev_unpacked);
    HC(hipEventRecord(ev_filled, ctx->stream));
    HC(hipStreamWaitEvent(ctx->stream2, ev_filled, 0));
    launch_unpack_supplied(ctx->stream2, cc, d_bytes, a.src, s->d_omit, R, d_sup_in, d_sup_corr, d_sup_rec, sup_nq);
    HC(hipEventRecord(ev_unpacked, ctx->stream2));
    ctx->phase(RV_PH_SETUP);
    ctx->count(2);
    launch_expand_seeds(ctx->stream, s->d_seeds, R, s->d_keys);
    launch_overlay_rows(ctx->stream, (uint32_t*)s->d_keys, (const uint32_t*)a.hkeys, s->d_omit, R, 32, 1);
    if (has64) {
        launch_expand_seeds(ctx->stream, a.seeds64, R, s->d_keys64);
        launch_overlay_rows(ctx->stream, (uint32_t*)s->d_keys64, (const uint32_t*)a.hkeys64, s->d_omit64, R, 32, 1);
        ctx->count(2);
    }
    ctx->phase(-1);
    // (the schedule switches of verify_groups_impl, without its conditions on how the proof was uploaded)
    s->z64f = has64 && c->z64f_ok && z64_fused_on() && z64_fused_supports(NQ) &&
              !(getenv("RV_Z64_FUSED_VERIFY") && atoi(getenv("RV_Z64_FUSED_VERIFY")) == 0);
    {
        const int head_pct = getenv("RV_VERIFY_HEAD") ? std::min(std::max(atoi(getenv("RV_VERIFY_HEAD")), 0), 100) : 65;
        const uint64_t n_blocks = cc.n_masks_pad / 128;
        const uint64_t ov_min = getenv("RV_OVERLAP_MIN") ? strtoull(getenv("RV_OVERLAP_MIN"), nullptr, 0) : 8192;
        const int ov_mode = getenv("RV_OVERLAP") ? atoi(getenv("RV_OVERLAP")) : 1;
        s->overlap = head_pct < 100 && ov_mode != 0 && aes_col4_supports(NQ) && n_blocks >= ov_min;
        s->ov_head = s->overlap ? n_blocks * (uint64_t)head_pct / 100 : 0;
    }
    if ((rc = shard_setup_prg(s, a.keep, a.keep64))) return fail(rc);
    HC(hipStreamWaitEvent(ctx->stream, ev_unpacked, 0));
    Interp64Params p64{};
    if (has64) {
        launch_unpack_supplied64(ctx->stream, cc, d_bytes, a.src64, s->d_omit64, R, d_sup_in64, d_sup_corr64, d_sup_rec64, sup_r);
        p64.omit = s->d_omit64;
        p64.sup_in = d_sup_in64;
        p64.sup_corr = d_sup_corr64;
        p64.sup_rec = d_sup_rec64;
        p64.sup_r = sup_r;
    }
    InterpParams p{};
    p.on_mask = a.onm;
    p.sup_in = d_sup_in;
    p.sup_corr = d_sup_corr;
    p.sup_rec = d_sup_rec;
    p.sup_nq = sup_nq;
    const bool vc_on = !(getenv("RV_VERIFY_VC") && atoi(getenv("RV_VERIFY_VC")) == 0);
    int vmode = MODE_VERIFY;
    if (vc_on && c->vclr_ok && !c->general_levels) {  // (MODE_VERIFY_C: a whole proof, every opened repetition in the first sixteen quad words)
        uint64_t* d_vc = nullptr;
        DA((size_t)cc.n_rows, d_vc);
        HC(hipMemsetAsync(d_vc + cc.zero_row, 0, 8, ctx->stream));
        p.vc = d_vc;
        vmode = MODE_VERIFY_C;
        g_verify_vc.fetch_add(1, std::memory_order_relaxed);
    }
    if ((rc = shard_run(s, vmode, p, p64))) return fail(rc);
    // preprocessing slots: the online commitment is the one carried by the proof (preprocess.rs:55-57)
    launch_overlay_rows(ctx->stream, s->d_dig + 1 * DW, (const uint32_t*)a.hco, s->d_omit, R, 8, 0);
    launch_overlay_rows(ctx->stream, s->d_dig + 3 * DW, (const uint32_t*)a.hco64, s->d_omit, R, 8, 0);
    if ((rc = shard_join(s))) return fail(rc);
    int dev_flags = 0;
    uint8_t* stage_dev = nullptr;
    if (ctx->h_stage && hipHostGetDevicePointer((void**)&stage_dev, ctx->h_stage, 0) != hipSuccess) {
        (void)hipGetLastError();
        stage_dev = nullptr;
    }
    if (stage_dev) {
        launch_store_words(ctx->stream, (const uint32_t*)s->d_h, R * 8, (uint32_t*)stage_dev, s->d_err, (int*)(stage_dev + (size_t)R * 32));
        HC(hipStreamSynchronize(ctx->stream));
        memcpy(digests, ctx->h_stage, (size_t)R * 32);
        memcpy(&dev_flags, ctx->h_stage + (size_t)R * 32, sizeof dev_flags);
    } else {
        HC(hipMemcpyAsync(digests, s->d_h, (size_t)R * 32, hipMemcpyDeviceToHost, ctx->stream));
        HC(hipMemcpyAsync(&dev_flags, s->d_err, sizeof dev_flags, hipMemcpyDeviceToHost, ctx->stream));
        HC(hipStreamSynchronize(ctx->stream));
    }
    *zero_checks_ok = !(dev_flags & RV_DEV_ZERO_CHECK);
    ctx->collect();
    ctx->prof.calls++;
#undef HC
#undef DA
    rv_shard_destroy(s);
    return RV_OK;
}

// d_bytes[0, len) in one of the two framings (lens: the four section lengths, else null); comm_in: the sections form's
// commitment.  The answer of rv_verify_ex on the bincode(Proof) bytes the input stands for.
static int verify_device_impl(rv_ctx* ctx, const rv_circuit* c, const uint8_t* comm_in, const uint8_t* d_bytes, size_t len, const size_t* lens,
                              uint32_t flags, int* ok) {
    LibBusy busy_guard;  // (compile.h: the background unmapper keeps still while the GPU is driven)
    const int framing = lens ? VW_FRAMING_SECTIONS : VW_FRAMING_PROOF;
    *ok = 0;
    HIPCHK(hipSetDevice(ctx->device));
    if (int rb = device_bytes_ok(ctx, d_bytes, len, 16)) return rb;
    if (int rs2 = ctx_stream2(ctx)) return rs2;
    // ---- the walk and its 120 bytes back
    uint64_t* d_table = nullptr;
    int rc = dalloc(ctx, (size_t)VW_WORDS + 4, &d_table);
    if (rc) return rc;
    struct Release {
        rv_ctx* ctx;
        void* p;
        ~Release() { ctx->release(p); }  // (every path below has drained the streams that read it)
    } release_table{ctx, d_table};
    uint64_t* d_lens = nullptr;
    uint64_t lens64[4] = {0, 0, 0, 0};
    if (lens) {
        for (int i = 0; i < 4; i++) lens64[i] = lens[i];
        d_lens = d_table + VW_WORDS;
        HIPCHK(hipMemcpyAsync(d_lens, lens64, sizeof lens64, hipMemcpyHostToDevice, ctx->stream));
    }
    uint64_t head[VW_HEAD_WORDS];
    uint8_t* stage_dev = nullptr;
    if (!ctx->h_stage && hipHostMalloc((void**)&ctx->h_stage, rv_ctx::STAGE_BYTES, hipHostMallocMapped) != hipSuccess) {
        (void)hipGetLastError();
        ctx->h_stage = nullptr;
    }
    if (ctx->h_stage && hipHostGetDevicePointer((void**)&stage_dev, ctx->h_stage, 0) != hipSuccess) {
        (void)hipGetLastError();
        stage_dev = nullptr;
    }
    launch_parse_proof(ctx->stream, d_bytes, len, framing, d_lens, d_table, (uint64_t*)stage_dev);
    HIPCHK(hipGetLastError());
    if (!stage_dev) HIPCHK(hipMemcpyAsync(head, d_table + VW_HEAD, sizeof head, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    if (stage_dev) memcpy(head, ctx->h_stage, sizeof head);
    if (head[0] != (uint64_t)VW_OK) {
        // ---- not a well-framed proof of acceptable records: the host verifier's answer on a host copy
        g_verify_dev_paths[1].fetch_add(1, std::memory_order_relaxed);
        std::vector<uint8_t> h;
        if (!lens) {
            h.resize(std::max<size_t>(len, 1));
            if (len) HIPCHK(hipMemcpy(h.data(), d_bytes, len, hipMemcpyDeviceToHost));
            return rv_verify_impl(ctx, c, h.data(), len, flags, ok);
        }
        // comm | LE64(40) | sec0 | LE64(216) | sec1 | LE64(40) | sec2 | LE64(216) | sec3
        h.resize(32 + 4 * 8 + len);
        memcpy(h.data(), comm_in, 32);
        size_t at = 32, from = 0;
        for (int i = 0; i < 4; i++) {
            put_le64(h.data() + at, i % 2 ? RV_PREPROCESSING_REPS : RV_ONLINE_REPS);
            at += 8;
            if (lens[i]) HIPCHK(hipMemcpy(h.data() + at, d_bytes + from, lens[i], hipMemcpyDeviceToHost));
            at += lens[i];
            from += lens[i];
        }
        return rv_verify_impl(ctx, c, h.data(), h.size(), flags, ok);
    }
    g_verify_dev_paths[0].fetch_add(1, std::memory_order_relaxed);
    // (head is this call's copy: the staging buffer is written again by the digests' way out)
    const uint8_t* rec_omit = (const uint8_t*)(head + (VW_OMIT - VW_HEAD));
    const uint8_t* comm = lens ? comm_in : (const uint8_t*)(head + (VW_COMM - VW_HEAD));
    std::vector<uint8_t> dig((size_t)RV_TOTAL_REPS * 32);
    int zc = 1;
    if ((rc = verify_device_slots(ctx, c, d_bytes, d_table, dig.data(), &zc))) return rc;
    // ---- rv_verify_finish_impl's decision, from comm and the omit bytes the walk brought
    uint8_t omit[RV_TOTAL_REPS];
    *ok = digests_give_comm(comm, dig.data(), omit);
    if (verify_is_strict(flags)) {
        if (!zc) *ok = 0;
        if (!records_omit_challenge(omit, rec_omit, rec_omit + RV_ONLINE_REPS)) *ok = 0;
    }
    return RV_OK;
}

extern "C" int rv_verify_device(rv_ctx* ctx, const rv_circuit* c, const uint8_t* d_proof, size_t proof_len, uint32_t flags, int* ok) {
    if (!ctx || !c || !d_proof || !ok || !verify_flags_ok(flags)) return RV_E_ARG;
    return guarded([&] { return verify_device_impl(ctx, c, nullptr, d_proof, proof_len, nullptr, flags, ok); });
}

extern "C" int rv_verify_sections_device(rv_ctx* ctx, const rv_circuit* c, const uint8_t comm[RV_HASH_SIZE], const uint8_t* d_sections,
                                         const size_t lens[4], uint32_t flags, int* ok) {
    if (!ctx || !c || !comm || !d_sections || !lens || !ok || !verify_flags_ok(flags)) return RV_E_ARG;
    size_t total = 0;
    for (int i = 0; i < 4; i++) {
        if (lens[i] > SIZE_MAX - 64 - total) return RV_E_ARG;  // (no buffer is that long; the framed copy adds 64 bytes)
        total += lens[i];
    }
    return guarded([&] { return verify_device_impl(ctx, c, comm, d_sections, total, lens, flags, ok); });
}
