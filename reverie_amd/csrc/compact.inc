// Part of api.hip (#included there, one translation unit): rv_ops_compact_wires_device -- the wire compaction of compact_dev.hip on the
// context's stream, its work memory from the context arena -- and rv_compactor_*, the same for a list read in windows (compact_win.hip).
// (rv_ops_compact_wires, the host sweep, is compact.cpp.)

extern "C" int rv_ops_compact_wires_device(rv_ctx* ctx, const rv_op* d_ops, size_t n_ops, size_t z64_wires, size_t gf2_wires, rv_op* d_out,
                                           rv_compact_info* info) {
    if (!ctx || (n_ops && (!d_ops || !d_out))) return RV_E_ARG;
    if (n_ops >= (1ull << 31)) return RV_E_UNSUPPORTED;
    return guarded([&]() -> int {
        if (n_ops) {
            HIPCHK(hipSetDevice(ctx->device));
            if (int rb = device_bytes_ok(ctx, d_ops, n_ops * sizeof(rv_op), 8)) return rb;
            if (int rb = device_bytes_ok(ctx, d_out, n_ops * sizeof(rv_op), 8)) return rb;
            // (d_out == d_ops is the in-place form; any other overlap would have one thread read what another wrote)
            const uint8_t *i0 = (const uint8_t*)d_ops, *o0 = (const uint8_t*)d_out;
            if (o0 != i0 && o0 < i0 + n_ops * sizeof(rv_op) && i0 < o0 + n_ops * sizeof(rv_op)) return RV_E_ARG;
        }
        return stage_code(compact_ops_device(ctx->stream, ctx_dev_allocator(ctx), d_ops, n_ops, z64_wires, gf2_wires, d_out, info),
                          "device wire compaction");
    });
}

// ---- rv_compactor_*: the same compaction for a list read in windows (compact_win.hip), on the context's stream and arena ----
struct rv_compactor {
    rv_ctx* ctx;
    WinCompactor* w;
};

extern "C" int rv_compactor_begin(rv_ctx* ctx, size_t z64_wires, size_t gf2_wires, rv_compactor** out) {
    if (!ctx || !out) return RV_E_ARG;
    *out = nullptr;
    return guarded([&]() -> int {
        LibBusy busy_guard;
        HIPCHK(hipSetDevice(ctx->device));
        std::unique_ptr<rv_compactor> c(new rv_compactor{ctx, nullptr});
        const int rc = wincompact_begin(ctx->stream, ctx_dev_allocator(ctx), z64_wires, gf2_wires, &c->w);
        if (rc) return stage_code(rc, "windowed wire compaction");
        *out = c.release();
        return RV_OK;
    });
}

extern "C" void rv_compactor_destroy(rv_compactor* c) {
    if (!c) return;
    (void)hipSetDevice(c->ctx->device);
    wincompact_destroy(c->w);
    delete c;
}

// a scan feed (d_out null) or a rewrite feed (in place where d_out is a device `ops`)
static int compactor_pass(rv_compactor* c, const rv_op* ops, size_t n_ops, int ops_on_device, rv_op* d_out, bool rewrite) {
    const PassShape shape = {"windowed wire compaction", "windowed wire compaction: the pass is not the list that was scanned", rewrite, true, n_ops,
                             nullptr};
    return stage_pass(
        c ? c->ctx : nullptr, shape, ops, n_ops, ops_on_device, d_out,
        [&] { return rewrite ? wincompact_admit_feed(c->w, n_ops) : wincompact_admit_scan(c->w, n_ops); },
        [&](const rv_op* d_ops, size_t up_bytes) {
            return rewrite ? wincompact_feed(c->w, d_ops, n_ops, d_out, up_bytes) : wincompact_scan(c->w, d_ops, n_ops, up_bytes);
        });
}

extern "C" int rv_compactor_scan(rv_compactor* c, const rv_op* ops, size_t n_ops, int ops_on_device) {
    return compactor_pass(c, ops, n_ops, ops_on_device, nullptr, false);
}

extern "C" int rv_compactor_feed(rv_compactor* c, const rv_op* ops, size_t n_ops, int ops_on_device, rv_op* d_out) {
    return compactor_pass(c, ops, n_ops, ops_on_device, d_out, true);
}

extern "C" int rv_compactor_scan_end(rv_compactor* c, int* again, rv_compact_info* info) {
    if (!c || !again) return RV_E_ARG;
    return guarded([&]() -> int {
        LibBusy busy_guard;
        HIPCHK(hipSetDevice(c->ctx->device));
        return stage_code(wincompact_scan_end(c->w, again, info), "windowed wire compaction");
    });
}

extern "C" int rv_compactor_rewind(rv_compactor* c) {
    if (!c) return RV_E_ARG;
    return guarded([&]() -> int {
        LibBusy busy_guard;
        HIPCHK(hipSetDevice(c->ctx->device));
        return wincompact_rewind(c->w);
    });
}

extern "C" int rv_compactor_get_info(const rv_compactor* c, rv_compactor_info* info) {
    if (!c || !info) return RV_E_ARG;
    return wincompact_info(c->w, info);
}
