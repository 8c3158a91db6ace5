// Part of api.hip (#included there, one translation unit, behind verify.inc): rv_verify_device / rv_verify_sections_device --
// Proof::verify on proof bytes in device memory (verify_dev.h: the walk, the table, the two kernels).
//
// The call: k_parse_proof walks the framing, the host waits for its status word (with comm and the 80 omit bytes: 120 bytes through
// the mapped staging buffer).  A good status: VerifyRun (verify.inc) with its device source -- k_fill_slots_dev writes the slot
// arrays, the unpack kernels read the caller's buffer in place -- and no proof byte crosses to the host.  Any other
// status: the bytes are copied to the host and rv_verify_ex answers, so the answer for bytes that are not a well-framed proof of
// acceptable records is the host verifier's by construction.
//
// Ordering: there is no upload to hide, so none of the host source's staging (blob, the side-stream copy, split64).  Everything
// runs on the context's stream except the three GF(2) unpack kernels, which go to the second stream behind the fill kernel and run
// beside the mask generator as they do for host bytes; the levels wait for their event.

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
    uint8_t* const stage_dev = ctx->stage_mapped();
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
    if ((rc = VerifyRun(ctx, c, RV_TOTAL_REPS, 0, nullptr, d_bytes, d_table).run(dig.data(), &zc))) return rc;
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
