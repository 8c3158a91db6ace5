// Part of api.hip (#included there, one translation unit, last): the entry points that read witnesses in device memory --
// rv_prove_wdev, rv_prove_device_wdev, rv_prove_batch_wdev, rv_prove_batch_device_wdev -- and rv_evaluate_batch_device, which also
// leaves its results there.
//
// Each prover validates the descriptor and calls the _impl function of its host-witness sibling with a WitSrc (api.hip) that says
// "device": the paths, the error codes and the proof bytes are the sibling's, only the kind of the copies that bring the witness to
// where the kernels read it differs (shard.inc: device-to-device behind the staged seeds, or into the separate allocation;
// batch.inc: the two strided 2-D copies).  The evaluator reads the witnesses in place: k_eval_wit and the Z64 Input gates take the
// caller's pointers and strides (eval.inc).

static bool ranges_overlap(const void* a, size_t na, const void* b, size_t nb) {
    const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
    return na && nb && x < y + nb && y < x + na;
}

// The descriptor of `batch` witnesses, checked against the circuit and the device before anything is launched (the header's rules;
// the context's device is current) -> the source the _impl functions take.  A batch of one ignores the strides.
static int wit_dev_src(rv_ctx* ctx, const rv_circuit* c, size_t batch, const rv_dev_witness* dw, WitSrc* out) {
    const Compiled& cc = c->cc;
    if (dw->n_gf2 < cc.n_in || dw->n_z64 < cc.n_in64) return RV_E_WITNESS_SHORT;
    if ((cc.n_in && !dw->gf2) || (cc.n_in64 && !dw->z64)) return RV_E_ARG;
    WitSrc w{dw->gf2, dw->n_gf2, batch > 1 ? dw->stride_gf2 : dw->n_gf2, dw->z64, dw->n_z64, batch > 1 ? dw->stride_z64 : dw->n_z64, true};
    if (w.stride_gf2 < w.n_gf2 || w.stride_z64 < w.n_z64) return RV_E_ARG;
    if ((w.stride_gf2 && batch > SIZE_MAX / w.stride_gf2) || (w.stride_z64 && batch > SIZE_MAX / 8 / w.stride_z64)) return RV_E_ARG;
    if (w.gf2 && w.n_gf2)
        if (int rb = device_bytes_ok(ctx, w.gf2, (batch - 1) * w.stride_gf2 + w.n_gf2, 1)) return rb;
    if (w.z64 && w.n_z64)
        if (int rb = device_bytes_ok(ctx, w.z64, ((batch - 1) * w.stride_z64 + w.n_z64) * 8, 8)) return rb;
    *out = w;
    return RV_OK;
}

// whether [p, p + len) meets one of the batch's witness ranges
static bool wit_overlaps(const WitSrc& w, size_t batch, const void* p, size_t len) {
    return (w.gf2 && ranges_overlap(w.gf2, (batch - 1) * w.stride_gf2 + w.n_gf2, p, len)) ||
           (w.z64 && ranges_overlap(w.z64, ((batch - 1) * w.stride_z64 + w.n_z64) * 8, p, len));
}

// bincode(Proof) bytes of one proof of the circuit (the same for every witness: 40 / 216 split)
static size_t proof_total_bytes(const rv_circuit* c) { return whole_proof_layout(c->cc).total; }

extern "C" int rv_prove_wdev(rv_ctx* ctx, const rv_circuit* c, const rv_dev_witness* dw, const uint8_t* seeds, uint8_t** proof, size_t* proof_len) {
    if (!ctx || !c || !dw || !proof || !proof_len) return RV_E_ARG;
    return guarded([&]() -> int {
        *proof = nullptr;
        *proof_len = 0;
        HIPCHK(hipSetDevice(ctx->device));
        WitSrc w;
        if (int rc = wit_dev_src(ctx, c, 1, dw, &w)) return rc;
        return rv_prove_impl(ctx, c, w, seeds, proof, proof_len);
    });
}

extern "C" int rv_prove_device_wdev(rv_ctx* ctx, const rv_circuit* c, const rv_dev_witness* dw, const uint8_t* seeds, void* dst_device,
                                    uint8_t comm[RV_HASH_SIZE], uint8_t omit[RV_TOTAL_REPS], size_t lens[4]) {
    if (!ctx || !c || !dw || !seeds || !dst_device || !comm || !omit || !lens) return RV_E_ARG;
    return guarded([&]() -> int {
        HIPCHK(hipSetDevice(ctx->device));
        WitSrc w;
        if (int rc = wit_dev_src(ctx, c, 1, dw, &w)) return rc;
        // (the four sections: a whole proof without comm and the four counts)
        if (wit_overlaps(w, 1, dst_device, proof_total_bytes(c) - 32 - 4 * 8)) return RV_E_ARG;
        return rv_prove_device_impl(ctx, c, w, seeds, dst_device, comm, omit, lens);
    });
}

extern "C" int rv_prove_batch_wdev(rv_ctx* ctx, const rv_circuit* c, size_t batch, const rv_dev_witness* dw, const uint8_t* seeds, uint8_t** proofs,
                                   size_t* proof_lens) {
    if (!ctx || !c || !batch || !dw || !proofs || !proof_lens) return RV_E_ARG;
    return guarded([&]() -> int {
        for (size_t b = 0; b < batch; b++) proofs[b] = nullptr, proof_lens[b] = 0;
        HIPCHK(hipSetDevice(ctx->device));
        WitSrc w;
        if (int rc = wit_dev_src(ctx, c, batch, dw, &w)) return rc;
        return rv_prove_batch_impl(ctx, c, batch, w, seeds, BatchDst{proofs, proof_lens, nullptr, 0});
    });
}

extern "C" int rv_prove_batch_device_wdev(rv_ctx* ctx, const rv_circuit* c, size_t batch, const rv_dev_witness* dw, const uint8_t* seeds,
                                          void* dst_device, size_t stride, size_t* proof_len) {
    if (!ctx || !c || !batch || !dw || !seeds || !dst_device || !proof_len) return RV_E_ARG;
    return guarded([&]() -> int {
        const size_t total = proof_total_bytes(c);
        *proof_len = total;
        if (((uintptr_t)dst_device & 255) || (stride & 255) || stride < total || batch > SIZE_MAX / stride) return RV_E_ARG;
        HIPCHK(hipSetDevice(ctx->device));
        if (int rb = device_bytes_ok(ctx, dst_device, batch * stride, 16)) return rb;
        WitSrc w;
        if (int rc = wit_dev_src(ctx, c, batch, dw, &w)) return rc;
        if (wit_overlaps(w, batch, dst_device, batch * stride)) return RV_E_ARG;
        return rv_prove_batch_impl(ctx, c, batch, w, seeds, BatchDst{nullptr, nullptr, (uint8_t*)dst_device, stride});
    });
}

extern "C" int rv_evaluate_batch_device(rv_ctx* ctx, const rv_circuit* c, size_t batch, const rv_dev_witness* dw, const uint32_t* sel_gf2,
                                        size_t n_sel_gf2, const uint32_t* sel_z64, size_t n_sel_z64, uint8_t* d_gf2_values, uint64_t* d_z64_values,
                                        rv_eval_status* d_status) {
    if (!ctx || !c || !batch || !dw || !d_status) return RV_E_ARG;
    return guarded([&]() -> int {
        const Compiled& cc = c->cc;
        if ((!sel_gf2 && n_sel_gf2) || (!sel_z64 && n_sel_z64) || batch > UINT32_MAX) return RV_E_ARG;
        // what the circuit and the lengths decide, in rv_evaluate_batch's order (the descriptor's pointers are looked at below)
        if (int rc = eval_args_ok(c, WitSrc{dw->gf2, dw->n_gf2, 0, dw->z64, dw->n_z64, 0, true}, d_gf2_values || d_z64_values)) return rc;
        // values per witness: the selection's length, or every wire
        const size_t n2 = !d_gf2_values ? 0 : sel_gf2 ? n_sel_gf2 : cc.wire_forms.size();
        const size_t n64 = !d_z64_values ? 0 : sel_z64 ? n_sel_z64 : cc.wire_ssa64.size();
        for (size_t i = 0; i < (d_gf2_values ? n_sel_gf2 : 0); i++)
            if (sel_gf2[i] >= cc.wire_forms.size()) return RV_E_WIRE_OOB;
        for (size_t i = 0; i < (d_z64_values ? n_sel_z64 : 0); i++)
            if (sel_z64[i] >= cc.wire_ssa64.size()) return RV_E_WIRE_OOB;
        if (n2 > UINT32_MAX || n64 > UINT32_MAX || (n2 && batch > SIZE_MAX / n2) || (n64 && batch > SIZE_MAX / 8 / n64)) return RV_E_ARG;
        HIPCHK(hipSetDevice(ctx->device));
        WitSrc w;
        if (int rc = wit_dev_src(ctx, c, batch, dw, &w)) return rc;
        if (int rb = device_bytes_ok(ctx, d_status, batch * sizeof(rv_eval_status), 16)) return rb;
        if (n2)
            if (int rb = device_bytes_ok(ctx, d_gf2_values, batch * n2, 1)) return rb;
        if (n64)
            if (int rb = device_bytes_ok(ctx, d_z64_values, batch * n64 * 8, 8)) return rb;
        if (wit_overlaps(w, batch, d_status, batch * sizeof(rv_eval_status)) || (n2 && wit_overlaps(w, batch, d_gf2_values, batch * n2)) ||
            (n64 && wit_overlaps(w, batch, d_z64_values, batch * n64 * 8)))
            return RV_E_ARG;
        // the selections to the device (indices, no witness and no result), released behind the call's one wait
        uint32_t* d_sel = nullptr;
        const size_t ns2 = n2 && sel_gf2 ? n2 : 0, ns64 = n64 && sel_z64 ? n64 : 0;
        if (ns2 + ns64) {
            if (int rc = dalloc(ctx, ns2 + ns64, &d_sel)) return rc;
            if ((ns2 && hipMemcpyAsync(d_sel, sel_gf2, ns2 * 4, hipMemcpyHostToDevice, ctx->stream) != hipSuccess) ||
                (ns64 && hipMemcpyAsync(d_sel + ns2, sel_z64, ns64 * 4, hipMemcpyHostToDevice, ctx->stream) != hipSuccess)) {
                ctx->release(d_sel);
                return hip_fail(hipGetLastError(), "rv_evaluate_batch_device (selection)", __FILE__, __LINE__);
            }
        }
        const int rc = rv_evaluate_batch_impl(ctx, c, batch, w,
                                              EvalDst{n2 ? d_gf2_values : nullptr, n64 ? d_z64_values : nullptr, d_status, n2, n64, true, ns2 ? d_sel : nullptr,
                                                      ns64 ? d_sel + ns2 : nullptr});
        if (rc) (void)hipStreamSynchronize(ctx->stream);  // (nothing of this call is in flight when its selection block is reused)
        ctx->release(d_sel);
        return rc;
    });
}
