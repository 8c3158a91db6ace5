// Part of api.hip (#included there, one translation unit): rv_verify_batch.

// ------------------------------------------------------------------------------------
// rv_verify_batch: many proofs of one circuit in one pass -- the verifier's counterpart of rv_prove_batch's fused path
// (circuits below the large-circuit threshold, GF(2) and Z64 gates counted together; larger ones verify proof after
// proof).  Per proof the host only parses the bincode framing and fills its slot of ONE page-locked staging slab (seeds, omitted players,
// masks, opened keys, carried-over commitments, source offsets and the proof bytes themselves), which goes to the
// device in one copy; the per-proof kernel strings are recorded and replayed once per batch (launch.h), the levels run
// through the batched interpreter kernels in verify mode, and the slot digests plus the zero-check flags come back in
// one copy each.  The final check (rv_verify_finish_ex) is host work per proof.
// ------------------------------------------------------------------------------------
// What the one-pass body (verify_batch_pass) verifies, `live` naming the proofs of the batch that take part.
// The host form: the proofs' bytes and what parse_proof made of them.  The device form (d_proofs set; batch_dev.inc):
// proofs that lie in device memory and whose walk ended VW_OK -- live_refs[k] has live proof k's bytes and its table in device
// memory, heads[b] is proof b's table tail (status, the 80 omit bytes, comm) on the host.
struct VerifyBatchSrc {
    const uint8_t* const* proofs;
    const size_t* proof_lens;
    const std::vector<Parsed>* P;
    size_t max_len;
    const uint8_t* const* d_proofs;
    const BatchProofRef* live_refs;
    const uint64_t* heads;
};
static int verify_batch_pass(rv_ctx* ctx, const rv_circuit* c, const std::vector<size_t>& live, const VerifyBatchSrc& src, uint32_t flags, int* ok);

// a one-pass chunk: what fits in half of the free device memory, at least two proofs, RV_BATCH_MAX at most (read at every call)
static int verify_batch_chunk(rv_ctx* ctx, const Compiled& cc, size_t* chunk_out) {
    const bool has64 = !cc.gates64.empty();
    size_t free_b = 0, total_b = 0;
    if (hipMemGetInfo(&free_b, &total_b) != hipSuccess) return RV_E_DEVICE;
    size_t per_proof = std::max<size_t>(cc.info.scratch_bytes + 3 * (size_t)std::max<uint64_t>({cc.n_in, cc.n_pre, cc.n_rec, 1}) * 256, 1);
    if (has64) per_proof += 3 * (size_t)std::max<uint64_t>({cc.n_in64, cc.n_corr64, cc.n_rec64, 1}) * 64 * 8 + (size_t)RV_TOTAL_REPS * 128;
    size_t chunk = std::min<size_t>(std::max<size_t>((free_b + ctx->cached_bytes) / 2 / per_proof, 2), 4096);
    if (const char* e = getenv("RV_BATCH_MAX")) chunk = std::min<size_t>(chunk, (size_t)std::max(atoi(e), 2));
    *chunk_out = chunk;
    return RV_OK;
}

static int rv_verify_batch_impl(rv_ctx* ctx, const rv_circuit* c, size_t batch, const uint8_t* const* proofs, const size_t* proof_lens,
                                uint32_t flags, int* ok) {
    LibBusy busy_guard;  // (compile.h: the background unmapper keeps still while the GPU is driven)
    if (!ctx || !c || !batch || !proofs || !proof_lens || !ok || !verify_flags_ok(flags)) return RV_E_ARG;
    for (size_t b = 0; b < batch; b++) {
        ok[b] = 0;
        if (!proofs[b]) return RV_E_ARG;
    }
    const Compiled& cc = c->cc;
    // ---- parse.  A proof that cannot be parsed, has the wrong repetition counts (`false`, proof/mod.rs:225-230) or online records
    // the verifier's slots cannot take (check_records) is a rejected proof (ok[b] = 0) and takes no further part, not a failed
    // call: one bad proof from an untrusted peer must not keep the others from being verified.  Non-zero return codes are left
    // to argument / device errors.
    std::vector<Parsed> P(batch);
    std::vector<size_t> live;  // indices of the proofs that go to the GPU
    size_t max_len = 0;
    for (size_t b = 0; b < batch; b++) {
        if (parse_proof(proofs[b], proof_lens[b], P[b]) != RV_OK || !format_ok(P[b]) || check_records_range(P[b], 0, RV_TOTAL_REPS) != RV_OK) continue;
        live.push_back(b);
        max_len = std::max(max_len, proof_lens[b]);
    }
    if (batch == 1 || live.size() < 2 || cc.gates.size() + cc.gates64.size() >= batch_big_gates()) {  // proof after proof
        for (size_t b : live) {
            const int rc = rv_verify_ex(ctx, c, proofs[b], proof_lens[b], flags, &ok[b]);
            if (rc == RV_E_PROOF_MALFORMED)
                ok[b] = 0;
            else if (rc)
                return rc;
        }
        return RV_OK;
    }
    HIPCHK(hipSetDevice(ctx->device));
    {  // a pass keeps one proof's working set resident per proof: larger batches run as consecutive chunks
        size_t chunk = 0;
        if (int rcc = verify_batch_chunk(ctx, cc, &chunk)) return rcc;
        if (batch > chunk) {
            for (size_t b0 = 0; b0 < batch; b0 += chunk) {
                const int rc = rv_verify_batch_impl(ctx, c, std::min(chunk, batch - b0), proofs + b0, proof_lens + b0, flags, ok + b0);
                if (rc) return rc;
            }
            return RV_OK;
        }
    }
    return verify_batch_pass(ctx, c, live, VerifyBatchSrc{proofs, proof_lens, &P, max_len, nullptr, nullptr, nullptr}, flags, ok);
}

static int verify_batch_pass(rv_ctx* ctx, const rv_circuit* c, const std::vector<size_t>& live, const VerifyBatchSrc& src, uint32_t flags, int* ok) {
    const Compiled& cc = c->cc;
    const bool has64 = !cc.gates64.empty();
    const bool dev = src.d_proofs != nullptr;  // (the slab made on the device, the proofs read where they lie)
    const uint8_t* const* proofs = src.proofs;
    const size_t* proof_lens = src.proof_lens;
    const size_t B = live.size();
    const uint32_t R = RV_TOTAL_REPS, NQ = R / 4;
    // ---- the staging slab: one slot per proof
    struct Slot {
        size_t seeds, omit, keep, onm, quads, hkeys, hco, hco64, src, seeds64, omit64, keep64, hkeys64, src64, proof, stride;
    } L{};
    {
        size_t o = 0;
        auto take = [&](size_t n) {
            const size_t at = o;
            o += (n + 255) & ~(size_t)255;
            return at;
        };
        L.seeds = take((size_t)R * 16);
        L.omit = take(R);
        L.keep = take((size_t)NQ * 4);
        L.onm = take((size_t)NQ * 4);
        L.quads = take((size_t)NQ * 4);
        L.hkeys = take((size_t)R * 128);
        L.hco = take((size_t)R * 32);
        L.hco64 = take((size_t)R * 32);
        L.src = take((size_t)6 * R * 8);
        // the Z64 side (empty for a pure GF(2) circuit): its own seeds, omitted players, kept streams, opened keys, source offsets
        L.seeds64 = take(has64 ? (size_t)R * 16 : 0);
        L.omit64 = take(has64 ? R : 0);
        L.keep64 = take(has64 ? (size_t)NQ * 4 : 0);
        L.hkeys64 = take(has64 ? (size_t)R * 128 : 0);
        L.src64 = take(has64 ? (size_t)6 * R * 8 : 0);
        L.proof = take(dev ? 0 : src.max_len);
        L.stride = o;
    }
    std::vector<rv_shard*> sh(B, nullptr);
    std::vector<void*> pinned_tmp, device_tmp;
    std::vector<LaunchRecorder> recs(B);
    for (auto& r : recs) r.batch = (unsigned)B;
    struct RecorderOff {
        ~RecorderOff() { g_recorder = nullptr; }
    } recorder_off;
    InterpParams* d_pp = nullptr;
    auto cleanup = [&](int code) {
        g_recorder = nullptr;
        (void)hipStreamSynchronize(ctx->stream);
        for (rv_shard* s : sh)
            if (s) {
                s->destroy();
                delete s;
            }
        ctx->release(d_pp);
        for (void* q : device_tmp) ctx->release(q);
        for (void* q : pinned_tmp) g_pinned.put(q);
        return code;
    };
    constexpr size_t HEAD = 256;  // (no slot pointer equals an arena block: the slabs are released exactly once)
    uint8_t* h_slab = nullptr;
    if (!dev) {
        h_slab = (uint8_t*)g_pinned.get(std::max<size_t>(L.stride * B, PinnedPool::MIN_BYTES));
        if (!h_slab) return cleanup(RV_E_NOMEM);
        pinned_tmp.push_back(h_slab);
    }
    uint8_t* d_slab = nullptr;
    int rc;
    if ((rc = dalloc(ctx, HEAD + L.stride * B, &d_slab))) return cleanup(rc);
    device_tmp.push_back(d_slab);
    uint8_t* d_out = nullptr;  // per proof: 256 x 32 digest bytes, then the device flag word
    const size_t out_stride = (size_t)R * 32 + 256;
    if ((rc = dalloc(ctx, HEAD + out_stride * B, &d_out))) return cleanup(rc);
    device_tmp.push_back(d_out);
    std::vector<uint32_t> n_quads(B, RV_ONLINE_REPS / 4);  // (the device form: slots 0 .. 39 are the opened ones, quad words 0 .. 9)
    auto fill = [&](size_t k) {
        const std::vector<Parsed>& P = *src.P;
        const size_t b = live[k];
        uint8_t* h = h_slab + k * L.stride;
        const SlotArrays a{h + L.seeds, h + L.omit, h + L.hkeys, h + L.hco, h + L.hco64, (uint32_t*)(h + L.keep), (uint32_t*)(h + L.onm),
                           (uint64_t*)(h + L.src), h + L.seeds64, h + L.omit64, h + L.hkeys64, (uint32_t*)(h + L.keep64), (uint64_t*)(h + L.src64)};
        fill_slots_range(P[b], proofs[b], 0, R, L.proof, has64, a);  // (src offsets into this proof's slot)
        n_quads[k] = opened_quads(a.onm, NQ, (uint32_t*)(h + L.quads));
        memcpy(h + L.proof, proofs[b], proof_lens[b]);
    };
    if (dev) {
        // the slot arrays from the walks' tables, proof k's into slot k (src offsets from the proof's own first byte)
        BatchProofRef* d_refs = nullptr;
        if ((rc = dalloc(ctx, B, &d_refs))) return cleanup(rc);
        device_tmp.push_back(d_refs);
        BatchProofRef* h_refs = (BatchProofRef*)g_pinned.get(std::max<size_t>(B * sizeof(BatchProofRef), PinnedPool::MIN_BYTES));
        if (!h_refs) return cleanup(RV_E_NOMEM);
        pinned_tmp.push_back(h_refs);
        memcpy(h_refs, src.live_refs, B * sizeof(BatchProofRef));
        if (hipMemcpyAsync(d_refs, h_refs, B * sizeof(BatchProofRef), hipMemcpyHostToDevice, ctx->stream) != hipSuccess) return cleanup(RV_E_DEVICE);
        BatchSlotLayout BL{};
        BL.seeds = L.seeds, BL.omit = L.omit, BL.keep = L.keep, BL.onm = L.onm, BL.quads = L.quads, BL.hkeys = L.hkeys, BL.hco = L.hco, BL.hco64 = L.hco64;
        BL.src = L.src, BL.seeds64 = L.seeds64, BL.omit64 = L.omit64, BL.keep64 = L.keep64, BL.hkeys64 = L.hkeys64, BL.src64 = L.src64, BL.stride = L.stride;
        launch_fill_slots_batch(ctx->stream, d_refs, (uint32_t)B, d_slab + HEAD, BL, has64);
        if (hipGetLastError() != hipSuccess) return cleanup(RV_E_DEVICE);
    } else {
        // host work per proof (a few hundred KB of copies each): shared by a few threads for large batches
        const size_t n_thr = B >= 32 ? std::min<size_t>({(size_t)8, B / 8, (size_t)std::max(1u, std::thread::hardware_concurrency())}) : 1;
        auto range = [&](size_t k0, size_t k1) {
            for (size_t k = k0; k < k1; k++) fill(k);
        };
        if (n_thr <= 1) {
            range(0, B);
        } else {
            std::vector<std::thread> th;
            th.reserve(n_thr);
            try {
                for (size_t t = 0; t < n_thr; t++) th.emplace_back(range, B * t / n_thr, B * (t + 1) / n_thr);
            } catch (...) {  // a thread could not be started: the ranges without one are done here
                for (size_t t = th.size(); t < n_thr; t++) range(B * t / n_thr, B * (t + 1) / n_thr);
            }
            for (auto& x : th) x.join();
        }
    }
    if (!dev && hipMemcpyAsync(d_slab + HEAD, h_slab, L.stride * B, hipMemcpyHostToDevice, ctx->stream) != hipSuccess) return cleanup(RV_E_DEVICE);
    // ---- per proof (recorded): keys, masks, supplied-value rows, buffers
    std::vector<InterpParams> pp(B);
    std::vector<Interp64Params> pp64(has64 ? B : 0);
    // the Z64 supplied values of the opened repetitions -- slots 0 .. 39 -- in rows of 64 (rv_verify_shard's sup_r for a whole proof)
    constexpr uint32_t SUP_R64 = 64;
    for (size_t k = 0; k < B && !rc; k++) {
        uint8_t* d = d_slab + HEAD + k * L.stride;
        const uint8_t* d_bytes = dev ? src.d_proofs[live[k]] : d;  // (what the src / src64 offsets count from)
        rv_shard* s = sh[k] = new rv_shard();
        s->ctx = ctx;
        s->c = c;
        s->rep_begin = 0;
        s->R = R;
        s->NQ = NQ;
        s->d_seeds = d + L.seeds;  // slab slots: not arena blocks, destroy() ignores them
        s->d_omit = d + L.omit;
        s->d_h = d_out + HEAD + k * out_stride;
        s->d_err = (int*)(d_out + HEAD + k * out_stride + (size_t)R * 32);
        s->d_on_quads = (const uint32_t*)(d + L.quads);
        s->n_on_quads = n_quads[k];
        if ((rc = dalloc(ctx, (size_t)R * 128, &s->d_keys))) break;
        uint32_t *d_sup_in = nullptr, *d_sup_corr = nullptr, *d_sup_rec = nullptr;
        if ((rc = dalloc(ctx, (size_t)std::max<uint64_t>(cc.n_in, 1) * NQ, &d_sup_in))) break;
        s->extra.push_back(d_sup_in);
        if ((rc = dalloc(ctx, (size_t)std::max<uint64_t>(cc.n_pre, 1) * NQ, &d_sup_corr))) break;
        s->extra.push_back(d_sup_corr);
        if ((rc = dalloc(ctx, (size_t)std::max<uint64_t>(cc.n_rec, 1) * NQ, &d_sup_rec))) break;
        s->extra.push_back(d_sup_rec);
        uint64_t *d_sup_in64 = nullptr, *d_sup_corr64 = nullptr, *d_sup_rec64 = nullptr;
        if (has64) {
            s->d_omit64 = d + L.omit64;
            if ((rc = dalloc(ctx, (size_t)R * 128, &s->d_keys64))) break;
            if ((rc = dalloc(ctx, (size_t)std::max<uint64_t>(cc.n_in64, 1) * SUP_R64, &d_sup_in64))) break;
            s->extra.push_back(d_sup_in64);
            if ((rc = dalloc(ctx, (size_t)std::max<uint64_t>(cc.n_corr64, 1) * SUP_R64, &d_sup_corr64))) break;
            s->extra.push_back(d_sup_corr64);
            if ((rc = dalloc(ctx, (size_t)std::max<uint64_t>(cc.n_rec64, 1) * SUP_R64, &d_sup_rec64))) break;
            s->extra.push_back(d_sup_rec64);
        }
        g_recorder = &recs[k];
        launch_verifier_keys(ctx->stream, R, s->d_seeds, d + L.hkeys, s->d_omit, s->d_keys);
        if (has64) launch_verifier_keys(ctx->stream, R, d + L.seeds64, d + L.hkeys64, s->d_omit64, s->d_keys64);
        // (k_z64_fused and the single verifier's side-stream schedule for the Z64 records -- ev_sup64, mid64 -- stay out: a fresh
        // shard's z64f is false, and the records are unpacked here, from the slot, on the main stream)
        if (!(rc = shard_setup_prg(s, (const uint32_t*)(d + L.keep), has64 ? (const uint32_t*)(d + L.keep64) : nullptr))) {
            launch_unpack_supplied(ctx->stream, cc, d_bytes, (const uint64_t*)(d + L.src), s->d_omit, R, d_sup_in, d_sup_corr, d_sup_rec, NQ);
            Interp64Params p64{};
            if (has64) {
                launch_unpack_supplied64(ctx->stream, cc, d_bytes, (const uint64_t*)(d + L.src64), s->d_omit64, R, d_sup_in64, d_sup_corr64, d_sup_rec64,
                                         SUP_R64);
                p64.omit = s->d_omit64;
                p64.sup_in = d_sup_in64;
                p64.sup_corr = d_sup_corr64;
                p64.sup_rec = d_sup_rec64;
                p64.sup_r = SUP_R64;
            }
            pp[k] = InterpParams{};
            pp[k].on_mask = (const uint32_t*)(d + L.onm);
            pp[k].sup_in = d_sup_in;
            pp[k].sup_corr = d_sup_corr;
            pp[k].sup_rec = d_sup_rec;
            pp[k].sup_nq = NQ;
            rc = shard_run_alloc(s, pp[k], p64);
            if (has64) pp64[k] = p64;
        }
        g_recorder = nullptr;
    }
    if (rc) return cleanup(rc);
    if ((rc = replay_recorded(ctx, recs, pinned_tmp, device_tmp))) return cleanup(rc);
    // ---- all proofs level by level, verify mode
    if ((rc = dalloc(ctx, B, &d_pp))) return cleanup(rc);
    if (hipMemcpyAsync(d_pp, pp.data(), B * sizeof(InterpParams), hipMemcpyHostToDevice, ctx->stream) != hipSuccess) return cleanup(RV_E_DEVICE);
    Interp64Params* d_pp64 = nullptr;
    if (has64) {
        if ((rc = dalloc(ctx, B, &d_pp64))) return cleanup(rc);
        device_tmp.push_back(d_pp64);
        if (hipMemcpyAsync(d_pp64, pp64.data(), B * sizeof(Interp64Params), hipMemcpyHostToDevice, ctx->stream) != hipSuccess) return cleanup(RV_E_DEVICE);
        ctx->phase(RV_PH_INTERP);  // (Z64 / mixed circuits: one count per batched launch, as in rv_prove_batch)
    }
    launch_levels_batched(ctx, c, MODE_VERIFY, d_pp, d_pp64, B);
    if (has64) ctx->phase(-1);
    // ---- per proof (recorded): digests, the commitments the preprocessing slots carry over, join
    for (size_t k = 0; k < B && !rc; k++) {
        uint8_t* d = d_slab + HEAD + k * L.stride;
        rv_shard* s = sh[k];
        g_recorder = &recs[k];
        if (!(rc = shard_run_hash(s))) {
            launch_carried_commitments(ctx->stream, s, d + L.hco, d + L.hco64);
            rc = shard_join(s);
        }
        g_recorder = nullptr;
    }
    if (rc) return cleanup(rc);
    if ((rc = replay_recorded(ctx, recs, pinned_tmp, device_tmp))) return cleanup(rc);
    uint8_t* h_out = (uint8_t*)g_pinned.get(std::max<size_t>(out_stride * B, PinnedPool::MIN_BYTES));
    if (!h_out) return cleanup(RV_E_NOMEM);
    pinned_tmp.push_back(h_out);
    if (hipMemcpyAsync(h_out, d_out + HEAD, out_stride * B, hipMemcpyDeviceToHost, ctx->stream) != hipSuccess ||
        hipStreamSynchronize(ctx->stream) != hipSuccess)
        return cleanup(hip_fail(hipGetLastError(), "verify batch sync", __FILE__, __LINE__));
    if (has64) ctx->collect();
    // ---- the final check per proof (proof/mod.rs:283-306)
    for (size_t k = 0; k < B; k++) {
        const size_t b = live[k];
        int dev_flags = 0;
        memcpy(&dev_flags, h_out + k * out_stride + (size_t)R * 32, sizeof dev_flags);
        if (dev) {  // (verify_device_impl's decision: comm and the records' omit bytes are what the walk brought)
            const uint64_t* head = src.heads + b * (size_t)VW_HEAD_WORDS;
            const uint8_t* rec_omit = (const uint8_t*)(head + (VW_OMIT - VW_HEAD));
            uint8_t omit[RV_TOTAL_REPS];
            ok[b] = digests_give_comm((const uint8_t*)(head + (VW_COMM - VW_HEAD)), h_out + k * out_stride, omit);
            if (verify_is_strict(flags) && ((dev_flags & RV_DEV_ZERO_CHECK) || !records_omit_challenge(omit, rec_omit, rec_omit + RV_ONLINE_REPS))) ok[b] = 0;
            continue;
        }
        if ((rc = rv_verify_finish_ex(proofs[b], proof_lens[b], h_out + k * out_stride, flags, !(dev_flags & RV_DEV_ZERO_CHECK), &ok[b])))
            return cleanup(rc);
    }
    ctx->prof.calls += B;
    return cleanup(RV_OK);
}

extern "C" int rv_verify_batch(rv_ctx* ctx, const rv_circuit* c, size_t batch, const uint8_t* const* proofs, const size_t* proof_lens,
                               uint32_t flags, int* ok) {
    try {  // no C++ exception may cross the C boundary
        return rv_verify_batch_impl(ctx, c, batch, proofs, proof_lens, flags, ok);
    } catch (...) {
        g_last_error = "out of host memory";
        return RV_E_NOMEM;
    }
}
