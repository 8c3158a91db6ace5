// Part of api.hip (#included there, one translation unit, behind verify_batch.inc): rv_prove_batch_device and
// rv_verify_batch_device -- the batch entry points for a caller whose proofs stay in device memory.
//
// The prover is rv_prove_batch_impl (batch.inc) with another destination: every proof's openings are written, framed, into the
// caller's buffer, k_frame_counts adds the repetition counts the host form patches into its copy, and the per-proof error words
// are all that crosses to the host.
//
// The verifier: k_parse_proofs walks every proof's framing in one launch, the host waits for the heads (120 bytes per proof:
// status, the 80 omit bytes, comm).  A proof whose walk did not end VW_OK is copied to the host and gets what the host batch
// verifier gives it -- its own parse decides, so the answer is the host's by construction.  The others are the batch's live
// proofs: verify_batch_pass (verify_batch.inc) with the slab made by k_fill_slots_batch and the unpack kernels reading every
// proof in place, or -- fewer than two of them, a batch of one, a circuit from the large-circuit threshold on -- one
// verify_device_impl after another.

static std::atomic<uint64_t> g_verify_batch_dev_paths[3];  // proofs that took {the one-pass device path, verify_device_impl, the host fallback}
extern "C" int rv_hook_verify_batch_device_paths(uint64_t out[3]) {
    if (!out) return RV_E_ARG;
    for (int i = 0; i < 3; i++) out[i] = g_verify_batch_dev_paths[i].load(std::memory_order_relaxed);
    return RV_OK;
}

extern "C" int rv_prove_batch_device(rv_ctx* ctx, const rv_circuit* c, size_t batch, const uint8_t* wit_gf2, size_t n_gf2, const uint64_t* wit_z64,
                                     size_t n_z64, const uint8_t* seeds, void* dst_device, size_t stride, size_t* proof_len) {
    if (!ctx || !c || !batch || !seeds || !dst_device || !proof_len) return RV_E_ARG;
    return guarded([&]() -> int {
        const size_t total = whole_proof_layout(c->cc).total;
        *proof_len = total;
        if (((uintptr_t)dst_device & 255) || (stride & 255) || stride < total || batch > SIZE_MAX / stride) return RV_E_ARG;
        HIPCHK(hipSetDevice(ctx->device));
        if (int rb = device_bytes_ok(ctx, dst_device, batch * stride, 16)) return rb;
        return rv_prove_batch_impl(ctx, c, batch, wit_host(wit_gf2, n_gf2, wit_z64, n_z64), seeds, BatchDst{nullptr, nullptr, (uint8_t*)dst_device, stride});
    });
}

// what rv_verify_batch gives a proof its parse, format_ok or check_records refuses -- ok = 0 -- decided by the host's own parse
// of a host copy; a proof the host would take after all (the walk and the parse then disagree) is verified from that copy
static int verify_batch_device_fallback(rv_ctx* ctx, const rv_circuit* c, const uint8_t* d_proof, size_t len, uint32_t flags, int* ok) {
    std::vector<uint8_t> h(std::max<size_t>(len, 1));
    if (len) HIPCHK(hipMemcpy(h.data(), d_proof, len, hipMemcpyDeviceToHost));
    *ok = 0;
    Parsed P;
    if (parse_proof(h.data(), len, P) != RV_OK || !format_ok(P) || check_records_range(P, 0, RV_TOTAL_REPS) != RV_OK) return RV_OK;
    const int rc = rv_verify_impl(ctx, c, h.data(), len, flags, ok);
    if (rc == RV_E_PROOF_MALFORMED) {
        *ok = 0;
        return RV_OK;
    }
    return rc;
}

static int rv_verify_batch_device_impl(rv_ctx* ctx, const rv_circuit* c, size_t batch, const uint8_t* const* d_proofs, const size_t* proof_lens,
                                       uint32_t flags, int* ok) {
    LibBusy busy_guard;  // (compile.h: the background unmapper keeps still while the GPU is driven)
    const Compiled& cc = c->cc;
    HIPCHK(hipSetDevice(ctx->device));
    for (size_t b = 0; b < batch; b++) ok[b] = 0;
    // ---- the walks and their heads back: the call's one early synchronisation
    std::vector<void*> device_tmp, pinned_tmp;
    auto cleanup = [&](int code) {
        (void)hipStreamSynchronize(ctx->stream);
        for (void* q : device_tmp) ctx->release(q);
        for (void* q : pinned_tmp) g_pinned.put(q);
        return code;
    };
    int rc;
    BatchProofRef* d_refs = nullptr;
    uint64_t *d_tables = nullptr, *d_heads = nullptr;
    if ((rc = dalloc(ctx, batch, &d_refs))) return cleanup(rc);
    device_tmp.push_back(d_refs);
    if ((rc = dalloc(ctx, batch * (size_t)VW_WORDS, &d_tables))) return cleanup(rc);
    device_tmp.push_back(d_tables);
    BatchProofRef* h_refs = (BatchProofRef*)g_pinned.get(std::max<size_t>(batch * sizeof(BatchProofRef), PinnedPool::MIN_BYTES));
    if (!h_refs) return cleanup(RV_E_NOMEM);
    pinned_tmp.push_back(h_refs);
    for (size_t b = 0; b < batch; b++) h_refs[b] = BatchProofRef{d_proofs[b], (uint64_t)proof_lens[b], d_tables + b * (size_t)VW_WORDS};
    const size_t head_bytes = batch * (size_t)VW_HEAD_WORDS * 8;
    std::vector<uint64_t> heads(batch * (size_t)VW_HEAD_WORDS);
    uint8_t* const stage_dev = head_bytes <= rv_ctx::STAGE_BYTES ? ctx->stage_mapped() : nullptr;
    uint64_t* h_heads = nullptr;  // (without the mapped buffer: a page-locked one, one copy)
    if (!stage_dev) {
        if ((rc = dalloc(ctx, batch * (size_t)VW_HEAD_WORDS, &d_heads))) return cleanup(rc);
        device_tmp.push_back(d_heads);
        h_heads = (uint64_t*)g_pinned.get(std::max<size_t>(head_bytes, PinnedPool::MIN_BYTES));
        if (!h_heads) return cleanup(RV_E_NOMEM);
        pinned_tmp.push_back(h_heads);
    }
    if (hipMemcpyAsync(d_refs, h_refs, batch * sizeof(BatchProofRef), hipMemcpyHostToDevice, ctx->stream) != hipSuccess) return cleanup(RV_E_DEVICE);
    launch_parse_proofs(ctx->stream, d_refs, (uint32_t)batch, d_tables, stage_dev ? (uint64_t*)stage_dev : d_heads);
    if (hipGetLastError() != hipSuccess) return cleanup(RV_E_DEVICE);
    if (!stage_dev && hipMemcpyAsync(h_heads, d_heads, head_bytes, hipMemcpyDeviceToHost, ctx->stream) != hipSuccess) return cleanup(RV_E_DEVICE);
    if (hipStreamSynchronize(ctx->stream) != hipSuccess) return cleanup(hip_fail(hipGetLastError(), "verify batch (walks)", __FILE__, __LINE__));
    // (this call's copy: the staging buffer is written again by a single proof's verifier)
    memcpy(heads.data(), stage_dev ? (const void*)ctx->h_stage : (const void*)h_heads, head_bytes);
    std::vector<size_t> live;
    for (size_t b = 0; b < batch; b++)
        if (heads[b * (size_t)VW_HEAD_WORDS] == (uint64_t)VW_OK) live.push_back(b);
    // ---- the proofs the walk stopped in: the host's answer, from a host copy each
    auto answer_stopped = [&]() -> int {
        for (size_t b = 0, k = 0; b < batch; b++) {
            if (k < live.size() && live[k] == b) {
                k++;
                continue;
            }
            g_verify_batch_dev_paths[2].fetch_add(1, std::memory_order_relaxed);
            if (int rf = verify_batch_device_fallback(ctx, c, d_proofs[b], proof_lens[b], flags, &ok[b])) return rf;
        }
        return RV_OK;
    };
    if (batch == 1 || live.size() < 2 || cc.gates.size() + cc.gates64.size() >= batch_big_gates()) {  // proof after proof
        if ((rc = answer_stopped())) return cleanup(rc);
        for (size_t b : live) {
            g_verify_batch_dev_paths[1].fetch_add(1, std::memory_order_relaxed);
            rc = verify_device_impl(ctx, c, nullptr, d_proofs[b], proof_lens[b], nullptr, flags, &ok[b]);
            if (rc == RV_E_PROOF_MALFORMED)
                ok[b] = 0;
            else if (rc)
                return cleanup(rc);
        }
        return cleanup(RV_OK);
    }
    {  // a pass keeps one proof's working set resident per proof: larger batches run as consecutive chunks, each with its own walks
        size_t chunk = 0;
        if ((rc = verify_batch_chunk(ctx, cc, &chunk))) return cleanup(rc);
        if (batch > chunk) {
            (void)cleanup(RV_OK);
            for (size_t b0 = 0; b0 < batch; b0 += chunk)
                if ((rc = rv_verify_batch_device_impl(ctx, c, std::min(chunk, batch - b0), d_proofs + b0, proof_lens + b0, flags, ok + b0))) return rc;
            return RV_OK;
        }
    }
    if ((rc = answer_stopped())) return cleanup(rc);
    std::vector<BatchProofRef> live_refs(live.size());
    for (size_t k = 0; k < live.size(); k++) live_refs[k] = h_refs[live[k]];
    g_verify_batch_dev_paths[0].fetch_add(live.size(), std::memory_order_relaxed);
    rc = verify_batch_pass(ctx, c, live, VerifyBatchSrc{nullptr, nullptr, nullptr, 0, d_proofs, live_refs.data(), heads.data()}, flags, ok);
    return cleanup(rc);
}

extern "C" int rv_verify_batch_device(rv_ctx* ctx, const rv_circuit* c, size_t batch, const uint8_t* const* d_proofs, const size_t* proof_lens,
                                      uint32_t flags, int* ok) {
    if (!ctx || !c || !batch || !d_proofs || !proof_lens || !ok || !verify_flags_ok(flags) || batch > 0x7FFFFFFFu) return RV_E_ARG;
    return guarded([&]() -> int {
        HIPCHK(hipSetDevice(ctx->device));
        for (size_t b = 0; b < batch; b++) {
            if (!d_proofs[b]) return RV_E_ARG;
            if (int rb = device_bytes_ok(ctx, d_proofs[b], proof_lens[b], 16)) return rb;
        }
        return rv_verify_batch_device_impl(ctx, c, batch, d_proofs, proof_lens, flags, ok);
    });
}
