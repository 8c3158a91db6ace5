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
