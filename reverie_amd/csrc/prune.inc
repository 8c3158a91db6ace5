// Part of api.hip (#included there, one translation unit, behind link.inc): rv_ops_prune_device -- the kernels of prune_dev.hip on the
// context's stream, their work memory from the context arena.  (rv_ops_prune, the host sweep and the definition, is prune.cpp.)

extern "C" int rv_hook_prune_limits(uint32_t out[5]) {
    if (!out) return RV_E_ARG;
    out[0] = PRUNE_WG;
    out[1] = PRUNE_SOLO_LIMIT;
    out[2] = PRUNE_LOOK_INTERVAL;
    out[3] = PRUNE_TILE;
    out[4] = prune_max_rounds();
    return RV_OK;
}

extern "C" int rv_hook_prune_launches(uint64_t out[4]) {
    if (!out) return RV_E_ARG;
    prune_launches(out);
    return RV_OK;
}

extern "C" int rv_ops_prune_device(rv_ctx* ctx, const rv_op* d_ops, size_t n_ops, size_t z64_wires, size_t gf2_wires, const uint32_t* outputs_gf2,
                                   size_t n_outputs_gf2, const uint32_t* outputs_z64, size_t n_outputs_z64, rv_op* d_out, size_t cap, size_t* n_out,
                                   uint32_t* d_old_index, rv_prune_info* info) {
    if (!ctx || (n_ops && !d_ops) || (n_outputs_gf2 && !outputs_gf2) || (n_outputs_z64 && !outputs_z64)) return RV_E_ARG;
    if (n_ops >= (1ull << 31)) return RV_E_UNSUPPORTED;
    if (cap > (size_t)-1 / sizeof(rv_op)) return RV_E_ARG;
    if (!d_out) d_old_index = nullptr, cap = 0;  // (the counting call writes nothing)
    return guarded([&]() -> int {
        LibBusy busy_guard;
        if (n_ops) {
            HIPCHK(hipSetDevice(ctx->device));
            if (int rb = device_bytes_ok(ctx, d_ops, n_ops * sizeof(rv_op), 8)) return rb;
            if (d_out && cap) {
                if (int rb = device_bytes_ok(ctx, d_out, cap * sizeof(rv_op), 8)) return rb;
                // (no in-place form here: a tile's stores land where another tile's records are still to be read)
                const uint8_t *i0 = (const uint8_t*)d_ops, *o0 = (const uint8_t*)d_out;
                if (o0 < i0 + n_ops * sizeof(rv_op) && i0 < o0 + cap * sizeof(rv_op)) return RV_E_ARG;
                if (d_old_index)
                    if (int rb = device_bytes_ok(ctx, d_old_index, cap * sizeof(uint32_t), 4)) return rb;
            }
        }
        const uint32_t* const outs[2] = {outputs_gf2, outputs_z64};
        const size_t n_outs[2] = {n_outputs_gf2, n_outputs_z64};
        const int rc = prune_ops_device(ctx->stream, ctx_dev_allocator(ctx), d_ops, n_ops, z64_wires, gf2_wires, outs, n_outs, d_out, cap, n_out,
                                        d_old_index, info);
        if (rc == RV_E_DEVICE) g_last_error = "device pruning: HIP error";
        if (rc == RV_E_NOMEM) g_last_error = "device pruning: out of device memory";
        return rc;
    });
}

// ---- rv_pruner_*: the same pruning for a list read in windows (prune_win.hip), on the context's stream and arena ----
struct rv_pruner {
    rv_ctx* ctx;
    WinPruner* w;
};

static int pruner_code(int rc) {
    if (rc == RV_E_DEVICE) g_last_error = "windowed pruning: HIP error";
    if (rc == RV_E_NOMEM) g_last_error = "windowed pruning: out of device memory";
    return rc;
}

extern "C" int rv_pruner_begin(rv_ctx* ctx, size_t z64_wires, size_t gf2_wires, const uint32_t* outputs_gf2, size_t n_outputs_gf2,
                               const uint32_t* outputs_z64, size_t n_outputs_z64, rv_pruner** out) {
    if (!ctx || !out || (n_outputs_gf2 && !outputs_gf2) || (n_outputs_z64 && !outputs_z64)) return RV_E_ARG;
    *out = nullptr;
    return guarded([&]() -> int {
        LibBusy busy_guard;
        HIPCHK(hipSetDevice(ctx->device));
        std::unique_ptr<rv_pruner> p(new rv_pruner{ctx, nullptr});
        const uint32_t* const outs[2] = {outputs_gf2, outputs_z64};
        const size_t n_outs[2] = {n_outputs_gf2, n_outputs_z64};
        if (const int rc = pruner_code(winprune_begin(ctx->stream, ctx_dev_allocator(ctx), z64_wires, gf2_wires, outs, n_outs, &p->w))) return rc;
        *out = p.release();
        return RV_OK;
    });
}

extern "C" void rv_pruner_destroy(rv_pruner* p) {
    if (!p) return;
    (void)hipSetDevice(p->ctx->device);
    winprune_destroy(p->w);
    delete p;
}

// a feed of pass `pass` (0 scan, 1 mark, 2 emit): the checks of the pointers, the upload of a host feed, the call
static int pruner_pass(rv_pruner* p, int pass, const rv_op* ops, size_t n_ops, int ops_on_device, rv_op* d_out, size_t cap, size_t* n_out,
                       uint32_t* d_old_index) {
    if (!p || (n_ops && (!ops || (pass == 2 && !d_out)))) return RV_E_ARG;
    if (n_ops > (size_t)-1 / sizeof(rv_op)) return RV_E_UNSUPPORTED;
    if (cap > (size_t)-1 / sizeof(rv_op)) return RV_E_ARG;
    rv_ctx* ctx = p->ctx;
    return guarded([&]() -> int {
        LibBusy busy_guard;
        HIPCHK(hipSetDevice(ctx->device));
        const size_t bytes = n_ops * sizeof(rv_op);
        // (asked first, and before the upload: a call out of order is RV_E_ARG whatever its pointers are, and moves nothing)
        if (const int rc = winprune_admit(p->w, pass, n_ops)) return rc;
        if (n_ops) {
            if (ops_on_device)
                if (int rb = device_bytes_ok(ctx, ops, bytes, 8)) return rb;
            if (pass == 2 && cap) {
                if (int rb = device_bytes_ok(ctx, d_out, cap * sizeof(rv_op), 8)) return rb;
                // (no in-place form: a tile's stores land where another tile's records are still to be read)
                const uint8_t *i0 = (const uint8_t*)ops, *o0 = (const uint8_t*)d_out;
                if (ops_on_device && o0 < i0 + bytes && i0 < o0 + cap * sizeof(rv_op)) return RV_E_ARG;
                if (d_old_index)
                    if (int rb = device_bytes_ok(ctx, d_old_index, cap * sizeof(uint32_t), 4)) return rb;
            }
        }
        // the uploaded copy of a host feed: given back on every way out, once the stream is idle
        struct Upload {
            rv_ctx* ctx;
            void* d = nullptr;
            ~Upload() {
                if (d) {
                    (void)hipStreamSynchronize(ctx->stream);
                    ctx->release(d);
                }
            }
        } up{ctx};
        const rv_op* d_ops = ops;
        if (n_ops && !ops_on_device) {
            if (ctx->alloc(bytes, &up.d) != RV_OK) return pruner_code(RV_E_NOMEM);
            if (hipMemcpyAsync(up.d, ops, bytes, hipMemcpyHostToDevice, ctx->stream) != hipSuccess) return pruner_code(RV_E_DEVICE);
            d_ops = (const rv_op*)up.d;
        }
        const size_t up_bytes = up.d ? bytes : 0;
        const int rc = pass == 0   ? winprune_scan(p->w, d_ops, n_ops, up_bytes)
                       : pass == 1 ? winprune_mark(p->w, d_ops, n_ops, up_bytes, n_out)
                                   : winprune_feed(p->w, d_ops, n_ops, up_bytes, d_out, cap, n_out, d_old_index);
        if (rc == RV_E_ARG && pass) g_last_error = "windowed pruning: the pass is not the list that was scanned, or the room is too small";
        return pruner_code(rc);
    });
}

extern "C" int rv_pruner_scan(rv_pruner* p, const rv_op* ops, size_t n_ops, int ops_on_device) {
    return pruner_pass(p, 0, ops, n_ops, ops_on_device, nullptr, 0, nullptr, nullptr);
}

extern "C" int rv_pruner_mark(rv_pruner* p, const rv_op* ops, size_t n_ops, int ops_on_device, size_t* n_kept_here) {
    return pruner_pass(p, 1, ops, n_ops, ops_on_device, nullptr, 0, n_kept_here, nullptr);
}

extern "C" int rv_pruner_feed(rv_pruner* p, const rv_op* ops, size_t n_ops, int ops_on_device, rv_op* d_out, size_t cap, size_t* n_out,
                              uint32_t* d_old_index) {
    return pruner_pass(p, 2, ops, n_ops, ops_on_device, d_out, cap, n_out, d_old_index);
}

extern "C" int rv_pruner_scan_end(rv_pruner* p) {
    if (!p) return RV_E_ARG;
    return guarded([&]() -> int {
        LibBusy busy_guard;
        HIPCHK(hipSetDevice(p->ctx->device));
        return pruner_code(winprune_scan_end(p->w));
    });
}

extern "C" int rv_pruner_mark_end(rv_pruner* p, rv_prune_info* info) {
    if (!p) return RV_E_ARG;
    return guarded([&]() -> int {
        LibBusy busy_guard;
        return winprune_mark_end(p->w, info);
    });
}

extern "C" int rv_pruner_rewind(rv_pruner* p) {
    if (!p) return RV_E_ARG;
    return guarded([&]() -> int {
        LibBusy busy_guard;
        return winprune_rewind(p->w);
    });
}

extern "C" int rv_pruner_get_info(const rv_pruner* p, rv_pruner_info* info) {
    if (!p || !info) return RV_E_ARG;
    return winprune_info(p->w, info);
}
