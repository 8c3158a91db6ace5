// Part of api.hip (#included there, one translation unit, behind prune.inc): rv_ops_fold_device -- the kernels of fold_dev.hip on the
// context's stream, their work memory from the context arena.  (rv_ops_fold, the host sweep and the definition, is fold.cpp.)

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
