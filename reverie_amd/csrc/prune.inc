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
        const int rc = winprune_begin(ctx->stream, ctx_dev_allocator(ctx), z64_wires, gf2_wires, outs, n_outs, &p->w);
        if (rc) return stage_code(rc, "windowed pruning");
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

// a feed of pass `pass` (0 scan, 1 mark, 2 emit; no in-place form: the kept records close up)
static int pruner_pass(rv_pruner* p, int pass, const rv_op* ops, size_t n_ops, int ops_on_device, rv_op* d_out, size_t cap, size_t* n_out,
                       uint32_t* d_old_index) {
    const PassShape shape = {"windowed pruning", pass ? "windowed pruning: the pass is not the list that was scanned, or the room is too small" : nullptr,
                             pass == 2, false, cap, d_old_index};
    return stage_pass(
        p ? p->ctx : nullptr, shape, ops, n_ops, ops_on_device, d_out, [&] { return winprune_admit(p->w, pass, n_ops); },
        [&](const rv_op* d_ops, size_t up_bytes) {
            return pass == 0   ? winprune_scan(p->w, d_ops, n_ops, up_bytes)
                   : pass == 1 ? winprune_mark(p->w, d_ops, n_ops, up_bytes, n_out)
                               : winprune_feed(p->w, d_ops, n_ops, up_bytes, d_out, cap, n_out, d_old_index);
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
        return stage_code(winprune_scan_end(p->w), "windowed pruning");
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
