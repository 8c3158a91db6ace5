// Part of api.hip (#included there, one translation unit, behind prune.inc): rv_ops_fold_device and rv_folder_* -- the kernels of
// fold_dev.hip and fold_win.hip on the context's stream, their work memory from the context arena.  (rv_ops_fold, the host sweep and the definition, is fold.cpp.)

extern "C" int rv_hook_fold_limits(uint32_t out[5]) {
    if (!out) return RV_E_ARG;
    out[0] = FOLD_WG;
    out[1] = FOLD_SOLO_LIMIT;
    out[2] = FOLD_LOOK_INTERVAL;
    out[3] = FOLD_TILE;
    out[4] = fold_max_rounds();
    return RV_OK;
}

extern "C" int rv_hook_fold_launches(uint64_t out[4]) {
    if (!out) return RV_E_ARG;
    fold_launches(out);
    return RV_OK;
}

extern "C" int rv_ops_fold_device(rv_ctx* ctx, const rv_op* d_ops, size_t n_ops, size_t z64_wires, size_t gf2_wires, rv_op* d_out, rv_fold_info* info) {
    if (!ctx || (n_ops && !d_ops)) return RV_E_ARG;
    if (n_ops >= (1ull << 31)) return RV_E_UNSUPPORTED;
    return guarded([&]() -> int {
        LibBusy busy_guard;
        if (n_ops) {
            HIPCHK(hipSetDevice(ctx->device));
            if (int rb = device_bytes_ok(ctx, d_ops, n_ops * sizeof(rv_op), 8)) return rb;
            if (d_out && d_out != d_ops) {
                if (int rb = device_bytes_ok(ctx, d_out, n_ops * sizeof(rv_op), 8)) return rb;
                // (d_out == d_ops is the in-place form: a tile writes the records it read; any other overlap has a tile's stores
                // land where another tile's records are still to be read)
                const uint8_t *i0 = (const uint8_t*)d_ops, *o0 = (const uint8_t*)d_out;
                if (o0 < i0 + n_ops * sizeof(rv_op) && i0 < o0 + n_ops * sizeof(rv_op)) return RV_E_ARG;
            }
        }
        const int rc = fold_ops_device(ctx->stream, ctx_dev_allocator(ctx), d_ops, n_ops, z64_wires, gf2_wires, d_out, info);
        if (rc == RV_E_DEVICE) g_last_error = "device folding: HIP error";
        if (rc == RV_E_NOMEM) g_last_error = "device folding: out of device memory";
        return rc;
    });
}

// ---- rv_folder_*: the same folding for a list read in windows (fold_win.hip), on the context's stream and arena ----
struct rv_folder {
    rv_ctx* ctx;
    WinFolder* w;
};

extern "C" int rv_folder_begin(rv_ctx* ctx, size_t z64_wires, size_t gf2_wires, uint32_t flags, rv_folder** out) {
    if (!ctx || !out || (flags & ~(uint32_t)RV_FOLDER_KEEP_LOG)) return RV_E_ARG;
    *out = nullptr;
    return guarded([&]() -> int {
        LibBusy busy_guard;
        HIPCHK(hipSetDevice(ctx->device));
        std::unique_ptr<rv_folder> f(new rv_folder{ctx, nullptr});
        const int rc = winfold_begin(ctx->stream, ctx_dev_allocator(ctx), z64_wires, gf2_wires, (flags & RV_FOLDER_KEEP_LOG) != 0, &f->w);
        if (rc) return stage_code(rc, "windowed folding");
        *out = f.release();
        return RV_OK;
    });
}

extern "C" void rv_folder_destroy(rv_folder* f) {
    if (!f) return;
    (void)hipSetDevice(f->ctx->device);
    winfold_destroy(f->w);
    delete f;
}

// a feed (pass 0; d_out null: counted only) or a replay (pass 1), in place where d_out is a device `ops`
static int folder_pass(rv_folder* f, int pass, const rv_op* ops, size_t n_ops, int ops_on_device, uint64_t first, rv_op* d_out) {
    const PassShape shape = {"windowed folding", "windowed folding: the pass is not the list that was folded first", pass == 1, true, n_ops, nullptr};
    return stage_pass(
        f ? f->ctx : nullptr, shape, ops, n_ops, ops_on_device, d_out, [&] { return winfold_admit(f->w, pass, n_ops, first); },
        [&](const rv_op* d_ops, size_t up_bytes) {
            return pass == 0 ? winfold_feed(f->w, d_ops, n_ops, up_bytes, d_out) : winfold_replay(f->w, d_ops, n_ops, up_bytes, first, d_out);
        });
}

extern "C" int rv_folder_feed(rv_folder* f, const rv_op* ops, size_t n_ops, int ops_on_device, rv_op* d_out) {
    return folder_pass(f, 0, ops, n_ops, ops_on_device, 0, d_out);
}

extern "C" int rv_folder_replay(rv_folder* f, const rv_op* ops, size_t n_ops, int ops_on_device, uint64_t first_ordinal, rv_op* d_out) {
    return folder_pass(f, 1, ops, n_ops, ops_on_device, first_ordinal, d_out);
}

extern "C" int rv_folder_end(rv_folder* f, rv_fold_info* info) {
    if (!f) return RV_E_ARG;
    return guarded([&]() -> int {
        LibBusy busy_guard;
        return winfold_end(f->w, info);
    });
}

extern "C" int rv_folder_rewind(rv_folder* f) {
    if (!f) return RV_E_ARG;
    return guarded([&]() -> int {
        LibBusy busy_guard;
        HIPCHK(hipSetDevice(f->ctx->device));
        return stage_code(winfold_rewind(f->w), "windowed folding");
    });
}

extern "C" int rv_folder_replay_end(rv_folder* f) {
    if (!f) return RV_E_ARG;
    return guarded([&]() -> int {
        LibBusy busy_guard;
        return winfold_replay_end(f->w);
    });
}

extern "C" int rv_folder_get_info(const rv_folder* f, rv_folder_info* info) {
    if (!f || !info) return RV_E_ARG;
    return winfold_info(f->w, info);
}
