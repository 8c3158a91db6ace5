// Part of api.hip (#included there, one translation unit, behind eval_stream.inc): the streams' entry points for a caller whose
// witnesses and proofs live in device memory --
//   rv_stream_feed_wdev, rv_eval_stream_feed_wdev      witnesses read in device memory (ops from either side),
//   rv_stream_finish_device, _finish_batch_device      the finished proof written, counts and all, into the caller's device buffer,
//   rv_stream_verify_begin_device, _begin_batch_device a streaming verifier over proof bytes that stay where they are,
// and the counters and the digest hook the tests read.  Each is its host sibling's _impl function (stream.inc, eval_stream.inc) with
// another source or destination: the chunks, the digests, the error codes and the proof bytes are the sibling's.

extern "C" int rv_hook_stream_traffic(uint64_t out[4]) {
    if (!out) return RV_E_ARG;
    for (int i = 0; i < 4; i++) out[i] = g_stream_traffic[i].load(std::memory_order_relaxed);
    return RV_OK;
}

static std::atomic<uint64_t> g_stream_verify_dev_paths[2];  // device begins that took {the in-place path, the host fallback}
extern "C" int rv_hook_stream_verify_device_paths(uint64_t out[2]) {
    if (!out) return RV_E_ARG;
    out[0] = g_stream_verify_dev_paths[0].load(std::memory_order_relaxed);
    out[1] = g_stream_verify_dev_paths[1].load(std::memory_order_relaxed);
    return RV_OK;
}

// wit_digest on the host, and k_wit_sums on a device copy of the same arrays (the GF(2) copy starts 3 bytes into its allocation:
// the kernel may not assume more than the byte alignment the entry points promise)
extern "C" int rv_hook_stream_wit_sums(rv_ctx* ctx, const uint8_t* gf2, size_t n_gf2, uint64_t first_gf2, const uint64_t* z64, size_t n_z64,
                                       uint64_t first_z64, uint64_t* host_out, uint64_t* dev_out) {
    return guarded([&]() -> int {
        if (!ctx || !host_out || !dev_out || (n_gf2 && !gf2) || (n_z64 && !z64)) return RV_E_ARG;
        HIPCHK(hipSetDevice(ctx->device));
        *host_out = wit_digest(gf2, n_gf2, first_gf2, z64, n_z64, first_z64);
        uint8_t* d2 = nullptr;
        uint64_t *d64 = nullptr, *d_acc = nullptr;
        int rc;
        if ((rc = dalloc(ctx, n_gf2 + 3, &d2)) || (rc = dalloc(ctx, std::max<size_t>(n_z64, 1), &d64)) || (rc = dalloc(ctx, 1, &d_acc))) {
            ctx->release(d2), ctx->release(d64), ctx->release(d_acc);
            return rc;
        }
        hipStream_t st = ctx->stream;
        bool ok = hipMemsetAsync(d_acc, 0, 8, st) == hipSuccess;
        ok = ok && (!n_gf2 || hipMemcpyAsync(d2 + 3, gf2, n_gf2, hipMemcpyHostToDevice, st) == hipSuccess);
        ok = ok && (!n_z64 || hipMemcpyAsync(d64, z64, n_z64 * 8, hipMemcpyHostToDevice, st) == hipSuccess);
        if (ok) launch_wit_sums(st, d2 + 3, 0, n_gf2, first_gf2, d64, 0, n_z64, first_z64, &d_acc, 1);
        ok = ok && hipGetLastError() == hipSuccess && hipMemcpyAsync(dev_out, d_acc, 8, hipMemcpyDeviceToHost, st) == hipSuccess;
        ok = (hipStreamSynchronize(st) == hipSuccess) && ok;
        ctx->release(d2), ctx->release(d64), ctx->release(d_acc);
        return ok ? RV_OK : hip_fail(hipGetLastError(), "rv_hook_stream_wit_sums", __FILE__, __LINE__);
    });
}

// The descriptor of a feed's witnesses for `batch` proofs, checked against the device before anything is launched: wit_dev_src's
// rules without a circuit (a stream learns chunk by chunk how many elements it consumes: RV_E_WITNESS_SHORT comes from there).
// A NULL descriptor stands for "no witness" (a verifier stream).  The context's device is current.
struct StreamWitDev {
    const uint8_t* gf2 = nullptr;
    size_t n_gf2 = 0, stride2 = 0;
    const uint64_t* z64 = nullptr;
    size_t n_z64 = 0, stride64 = 0;
};
static int stream_wit_dev(rv_ctx* ctx, size_t batch, const rv_dev_witness* dw, StreamWitDev* out) {
    *out = StreamWitDev{};
    if (!dw) return RV_OK;
    StreamWitDev w;
    w.gf2 = dw->gf2, w.n_gf2 = dw->n_gf2, w.stride2 = batch > 1 ? dw->stride_gf2 : dw->n_gf2;
    w.z64 = dw->z64, w.n_z64 = dw->n_z64, w.stride64 = batch > 1 ? dw->stride_z64 : dw->n_z64;
    if ((w.n_gf2 && !w.gf2) || (w.n_z64 && !w.z64)) return RV_E_ARG;
    if (w.stride2 < w.n_gf2 || w.stride64 < w.n_z64) return RV_E_ARG;
    if ((w.stride2 && batch > SIZE_MAX / w.stride2) || (w.stride64 && batch > SIZE_MAX / 8 / w.stride64)) return RV_E_ARG;
    if (w.n_gf2)
        if (int rb = device_bytes_ok(ctx, w.gf2, (batch - 1) * w.stride2 + w.n_gf2, 1)) return rb;
    if (w.n_z64)
        if (int rb = device_bytes_ok(ctx, w.z64, ((batch - 1) * w.stride64 + w.n_z64) * 8, 8)) return rb;
    if (!w.n_gf2) w.gf2 = nullptr;
    if (!w.n_z64) w.z64 = nullptr;
    *out = w;
    return RV_OK;
}

extern "C" int rv_stream_feed_wdev(rv_stream* S, const rv_op* ops, size_t n_ops, int ops_on_device, const rv_dev_witness* dw) {
    if (!S) return RV_E_ARG;
    const int rc = guarded([&]() -> int {
        if (S->sticky) return S->sticky;
        const bool verifier = S->pass == 3;
        if (verifier ? (dw && (dw->n_gf2 || dw->n_z64)) : !dw) return S->sticky = RV_E_ARG;
        HIPCHK(hipSetDevice(S->ctx->device));
        StreamWitDev w;
        if (int rv = stream_wit_dev(S->ctx, std::max<size_t>(S->bat.size(), 1), verifier ? nullptr : dw, &w)) return S->sticky = rv;
        return stream_feed_impl(S, ops, ops_on_device != 0, n_ops, WitnessRows{w.gf2, w.n_gf2, w.stride2, w.z64, w.n_z64, w.stride64, !verifier});
    });
    // (the feed's one wait: behind it neither the ops nor the witness rows are read any more -- every chunk's copies and its digest
    // kernel were queued in front of the chunk's own wait or of this one)
    const int rs = stream_feed_settle(S);
    return rc ? rc : rs;
}

extern "C" int rv_eval_stream_feed_wdev(rv_eval_stream* E, const rv_op* ops, size_t n_ops, int ops_on_device, const rv_dev_witness* dw) {
    if (!E) return RV_E_ARG;
    const int rc = guarded([&]() -> int {
        if (E->sticky) return E->sticky;
        if (!dw) return E->sticky = RV_E_ARG;
        HIPCHK(hipSetDevice(E->ctx->device));
        StreamWitDev w;
        if (int rv = stream_wit_dev(E->ctx, E->B, dw, &w)) return E->sticky = rv;
        return eval_stream_feed_impl(E, ops, ops_on_device != 0, n_ops, EvalWitRows{w.gf2, w.n_gf2, w.stride2, w.z64, w.n_z64, w.stride64, true});
    });
    if (rc == RV_E_NOMEM) E->sticky = rc;
    // (the host feeds do not wait for the GPU; this one must, once: the caller's rows feed copies queued by the chunks)
    if (hipStreamSynchronize(E->ctx->stream) != hipSuccess && !rc) return E->sticky = hip_fail(hipGetLastError(), "rv_eval_stream_feed_wdev", __FILE__, __LINE__);
    return rc;
}

// ---- proofs left in device memory
// The destination of one proof: RV_E_ARG unless it is `align`-aligned memory of the stream's device with `room` >= the proof's length
// (inside its allocation); *proof_len = the required length either way.  The stream is untouched: the caller may call again.
static int stream_device_dst_ok(rv_stream* S, const void* dst, size_t room, size_t align, size_t* proof_len) {
    const size_t total = S->L.total;
    *proof_len = total;
    if (room < total || ((uintptr_t)dst & (align - 1))) return RV_E_ARG;
    return device_bytes_ok(S->ctx, dst, room, 16);
}

static int stream_finish_device_impl(rv_stream* S, void* dst_device, size_t cap, size_t align, size_t* proof_len) {
    if (!S || !dst_device || !proof_len) return RV_E_ARG;
    *proof_len = 0;
    if (!S->bat.empty()) return RV_E_ARG;  // (rv_stream_finish_batch_device)
    if (S->sticky) return S->sticky;
    if (S->pass != 2) return RV_E_ARG;
    HIPCHK(hipSetDevice(S->ctx->device));
    if (int rc = stream_device_dst_ok(S, dst_device, cap, align, proof_len)) return rc;
    return stream_finish_impl(S, nullptr, proof_len, (uint8_t*)dst_device);
}

extern "C" int rv_stream_finish_device(rv_stream* S, void* dst_device, size_t cap, size_t* proof_len) {
    return guarded([&] { return stream_finish_device_impl(S, dst_device, cap, 16, proof_len); });
}

extern "C" int rv_stream_finish_batch_device(rv_stream* S, void* dst_device, size_t stride, size_t* proof_len) {
    return guarded([&]() -> int {
        if (!S || !dst_device || !proof_len) return RV_E_ARG;
        if (S->bat.empty()) return stream_finish_device_impl(S, dst_device, stride, 16, proof_len);
        *proof_len = 0;
        if (S->sticky) return S->sticky;
        if (S->pass != 2) return RV_E_ARG;
        const size_t B = S->bat.size();
        HIPCHK(hipSetDevice(S->ctx->device));
        // rv_prove_batch_device's rules, for the whole destination before any member finishes
        const size_t total = S->bat[0]->L.total;
        *proof_len = total;
        if (((uintptr_t)dst_device & 255) || (stride & 255) || stride < total || B > SIZE_MAX / stride) return RV_E_ARG;
        if (int rb = device_bytes_ok(S->ctx, dst_device, B * stride, 16)) return rb;
        for (size_t b = 0; b < B; b++) {
            size_t len = 0;
            // (pass 2 was not fed what pass 1 was, for this witness or the stream: no proof comes out)
            if (int rc = stream_finish_impl(S->bat[b], nullptr, &len, (uint8_t*)dst_device + b * stride)) return S->sticky = rc;
        }
        S->sticky = RV_E_ARG;  // a finished stream takes no further calls (rv_stream_abort releases it)
        return RV_OK;
    });
}

// ---- the streaming verifier over a proof in device memory
// One walk (k_parse_proof) and its table back -- offsets, lengths, the 80 omit bytes, comm: nothing else of the proof crosses to the
// host.  VW_OK: the slot arrays come from k_fill_slots_dev, the preprocessing seeds reach the stream's begin in device memory, the
// chunks' unpack kernels read the caller's buffer by the table's offsets (d_vproof = d_proof), and finish decides from the table's
// head.  Any other status: the bytes are copied to a host buffer the stream owns and the host form begins, with its codes.
// as_member: a member of a batch -- a refused proof is a member that runs nothing and answers `false` (stream_verify_member's rule).
static int stream_verify_begin_device_impl(rv_ctx* ctx, size_t z64_wires, size_t gf2_wires, const uint8_t* d_proof, size_t proof_len, size_t max_chunk_ops,
                                           bool as_member, rv_stream** out) {
    if (!ctx || !out || !d_proof) return RV_E_ARG;
    *out = nullptr;
    LibBusy busy_guard;
    HIPCHK(hipSetDevice(ctx->device));
    if (int rb = device_bytes_ok(ctx, d_proof, proof_len, 16)) return rb;
    constexpr uint32_t R = rv_stream::R, NQ = rv_stream::NQ;
    hipStream_t st = ctx->stream;
    std::vector<void*> tmp;  // device scratch of this call, and the verifier's arrays until the stream owns them
    auto release_tmp = [&] {
        for (void* p : tmp) ctx->release(p);
        tmp.clear();
    };
    auto fail = [&](int code) {
        (void)hipStreamSynchronize(st);
        release_tmp();
        return code;
    };
    int rc;
    uint64_t* d_table = nullptr;
    if ((rc = dalloc(ctx, (size_t)VW_WORDS, &d_table))) return rc;
    tmp.push_back(d_table);
    std::vector<uint64_t> table(VW_WORDS, 0);
    launch_parse_proof(st, d_proof, proof_len, VW_FRAMING_PROOF, nullptr, d_table, nullptr);
    if (hipGetLastError() != hipSuccess || hipMemcpyAsync(table.data() + VW_HEAD, d_table + VW_HEAD, (size_t)VW_HEAD_WORDS * 8, hipMemcpyDeviceToHost, st) != hipSuccess ||
        hipStreamSynchronize(st) != hipSuccess)
        return fail(hip_fail(hipGetLastError(), "streaming verifier (walk)", __FILE__, __LINE__));
    if (table[VW_STATUS] != (uint64_t)VW_OK) {
        // ---- not a well-framed proof of acceptable records: the host form on a host copy, which the stream keeps
        release_tmp();
        g_stream_verify_dev_paths[1].fetch_add(1, std::memory_order_relaxed);
        std::vector<uint8_t> h(std::max<size_t>(proof_len, 1));
        if (proof_len) HIPCHK(hipMemcpy(h.data(), d_proof, proof_len, hipMemcpyDeviceToHost));
        rv_stream* S = nullptr;
        rc = stream_verify_begin_impl(ctx, z64_wires, gf2_wires, h.data(), proof_len, max_chunk_ops, &S);
        if (rc == RV_E_PROOF_MALFORMED && as_member) {
            S = stream_dead_verifier(ctx, h.data(), proof_len);
            rc = RV_OK;
        }
        if (rc) return rc;
        S->own_proof = std::move(h);  // (the vector's buffer moves with it: h_proof, where the host form left it, stays valid)
        S->h_proof = S->own_proof.data();
        *out = S;
        return RV_OK;
    }
    g_stream_verify_dev_paths[0].fetch_add(1, std::memory_order_relaxed);
    // the offsets and lengths of the records (the host keeps the Z64 vectors' places: ChunkRun shifts them chunk by chunk)
    if (hipMemcpy(table.data(), d_table, (size_t)VW_HEAD * 8, hipMemcpyDeviceToHost) != hipSuccess)
        return fail(hip_fail(hipGetLastError(), "streaming verifier (table)", __FILE__, __LINE__));
    // ---- the slot arrays on the device, where stream_verify_begin_impl uploads them
    DevSlotArrays a{};
    uint8_t* d_keys64 = nullptr;
    if ((rc = stream_verifier_alloc(ctx, a, d_keys64, tmp))) return fail(rc);
    launch_fill_slots_dev(st, d_proof, d_table, true, a);
    if (hipGetLastError() != hipSuccess) return fail(RV_E_DEVICE);
    // the prover's begin gives the stream its buffers and the GF(2) keys of the preprocessing slots, from the seeds the kernel wrote
    rv_stream* S = nullptr;
    if ((rc = stream_begin_impl(ctx, z64_wires, gf2_wires, a.seeds, max_chunk_ops, &S, /*seeds_on_device=*/true))) return fail(rc);
    S->pass = 3;
    S->proof_len = proof_len;
    S->proof_in_place = true;
    S->d_vproof = const_cast<uint8_t*>(d_proof);
    memcpy(S->dev_rec_omit, table.data() + VW_OMIT, sizeof S->dev_rec_omit);
    memcpy(S->dev_comm, table.data() + VW_COMM, sizeof S->dev_comm);
    S->src64.assign((size_t)6 * R, 0);  // fill_slots' src64 from the table: a Z64 vector is cut to the whole words of its group's first record
    for (uint32_t r = 0; r < RV_ONLINE_REPS; r++) {
        const uint64_t* z = table.data() + VW_REC + 8 * (VW_N_ON + r);
        const uint64_t* z0 = table.data() + VW_REC + 8 * (VW_N_ON + (r & ~7u));
        const int off[3] = {VW_OFF_REC, VW_OFF_CORR, VW_OFF_IN}, len[3] = {VW_LEN_REC, VW_LEN_CORR, VW_LEN_IN};
        for (int v = 0; v < 3; v++) {
            S->src64[(size_t)(2 * v) * R + r] = z[off[v]];
            S->src64[(size_t)(2 * v + 1) * R + r] = std::min(z[len[v]], z0[len[v]] / 8 * 8);
        }
    }
    // (the slot order puts the opened repetitions into the first ten quad words / forty repetitions: supplied_nq, supplied_r64)
    S->sup_nq = std::min(NQ, 16u);
    S->sup_r = std::min(R, 64u);
    if ((rc = stream_verifier_arm(S, a, d_keys64, tmp))) {
        rc = fail(rc);  // (waits, and releases the arrays the stream has not taken)
        rv_stream_abort(S);
        return rc;
    }
    release_tmp();
    *out = S;
    return RV_OK;
}


extern "C" int rv_stream_verify_begin_device(rv_ctx* ctx, size_t z64_wires, size_t gf2_wires, const uint8_t* d_proof, size_t proof_len, size_t max_chunk_ops,
                                             rv_stream** out) {
    return guarded([&] { return stream_verify_begin_device_impl(ctx, z64_wires, gf2_wires, d_proof, proof_len, max_chunk_ops, false, out); });
}

extern "C" int rv_stream_verify_begin_batch_device(rv_ctx* ctx, size_t z64_wires, size_t gf2_wires, size_t batch, const uint8_t* const* d_proofs,
                                                   const size_t* proof_lens, size_t max_chunk_ops, rv_stream** out) {
    return guarded([&]() -> int {
        if (!ctx || !out || !d_proofs || !proof_lens) return RV_E_ARG;
        *out = nullptr;
        if (!batch) return RV_E_ARG;
        for (size_t b = 0; b < batch; b++)
            if (!d_proofs[b]) return RV_E_ARG;
        if (gf2_wires > 0x3FFFFFFFull || z64_wires > 0x3FFFFFFFull) return RV_E_UNSUPPORTED;
        HIPCHK(hipSetDevice(ctx->device));
        auto begin = [&](size_t b, rv_stream** m) {
            return stream_verify_begin_device_impl(ctx, z64_wires, gf2_wires, d_proofs[b], proof_lens[b], max_chunk_ops, true, m);
        };
        if (batch == 1) return begin(0, out);
        return stream_batch_handle(ctx, z64_wires, gf2_wires, batch, 3, begin, out);
    });
}
