// Part of api.hip (#included there, one translation unit): rv_ops_compact_wires_device -- the wire compaction of compact_dev.hip on the
// context's stream, its work memory from the context arena.  (rv_ops_compact_wires, the host sweep, is compact.cpp.)

extern "C" int rv_ops_compact_wires_device(rv_ctx* ctx, const rv_op* d_ops, size_t n_ops, size_t z64_wires, size_t gf2_wires, rv_op* d_out,
                                           rv_compact_info* info) {
    if (!ctx || (n_ops && (!d_ops || !d_out))) return RV_E_ARG;
    if (n_ops >= (1ull << 31)) return RV_E_UNSUPPORTED;
    try {
        if (n_ops) {
            HIPCHK(hipSetDevice(ctx->device));
            if (int rb = device_bytes_ok(ctx, d_ops, n_ops * sizeof(rv_op), 8)) return rb;
            if (int rb = device_bytes_ok(ctx, d_out, n_ops * sizeof(rv_op), 8)) return rb;
            // (d_out == d_ops is the in-place form; any other overlap would have one thread read what another wrote)
            const uint8_t *i0 = (const uint8_t*)d_ops, *o0 = (const uint8_t*)d_out;
            if (o0 != i0 && o0 < i0 + n_ops * sizeof(rv_op) && i0 < o0 + n_ops * sizeof(rv_op)) return RV_E_ARG;
        }
        const int rc = compact_ops_device(ctx->stream, ctx_dev_allocator(ctx), d_ops, n_ops, z64_wires, gf2_wires, d_out, info);
        if (rc == RV_E_DEVICE) g_last_error = "device wire compaction: HIP error";
        if (rc == RV_E_NOMEM) g_last_error = "device wire compaction: out of device memory";
        return rc;
    } catch (...) {
        g_last_error = "out of host memory";
        return RV_E_NOMEM;
    }
}
