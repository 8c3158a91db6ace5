// Part of api.hip (#included there, one translation unit, behind verify_dev.inc): rv_link_plan_* -- the kernels of link_dev.hip on the
// context's stream, the plan's arrays in the context arena.  (rv_link, the host definition, is link.cpp.)

extern "C" int rv_hook_link_tiles(uint32_t out[2]) {
    if (!out) return RV_E_ARG;
    out[0] = LINK_TILE;
    out[1] = LINK_SCAN_BLOCK;
    return RV_OK;
}

struct rv_link_plan {
    rv_ctx* ctx;
    LinkPlan* p;
};

extern "C" int rv_link_plan_create(rv_ctx* ctx, const rv_link_desc* desc, uint32_t flags, rv_link_plan** plan) {
    if (!ctx || !plan) return RV_E_ARG;
    *plan = nullptr;
    if (flags & ~(RV_LINK_BLOCKS_ON_DEVICE | RV_LINK_TABLES_ON_DEVICE)) return RV_E_ARG;
    return guarded([&]() -> int {
        LibBusy busy_guard;
        uint64_t block_ops = 0;
        if (const int rc = lk_check_args(desc, &block_ops)) return rc;
        HIPCHK(hipSetDevice(ctx->device));
        if (flags & RV_LINK_BLOCKS_ON_DEVICE)
            for (uint64_t b = 0; b < desc->n_blocks; b++)
                if (desc->blocks[b].n_ops)
                    if (int rb = device_bytes_ok(ctx, desc->blocks[b].ops, desc->blocks[b].n_ops * sizeof(rv_op), 8)) return rb;
        if (flags & RV_LINK_TABLES_ON_DEVICE) {
            if (desc->n_instances)
                if (int rb = device_bytes_ok(ctx, desc->block_of, desc->n_instances * sizeof(uint32_t), 4)) return rb;
            if (desc->n_bindings)
                if (int rb = device_bytes_ok(ctx, desc->bindings, desc->n_bindings * sizeof(uint32_t), 4)) return rb;
        }
        std::unique_ptr<rv_link_plan> h(new rv_link_plan{ctx, nullptr});
        int code = RV_OK;
        rv_link_info info;
        const int rc = link_plan_create(ctx->stream, ctx_dev_allocator(ctx), desc, block_ops, flags, &code, &h->p, &info);
        if (rc == RV_E_DEVICE) g_last_error = "device linker: HIP error";
        if (rc == RV_E_NOMEM) g_last_error = "device linker: out of device memory";
        if (rc) return rc;
        if (code) return code;
        *plan = h.release();
        return RV_OK;
    });
}

extern "C" int rv_link_plan_info(const rv_link_plan* plan, rv_link_info* info) {
    if (!plan || !info) return RV_E_ARG;
    *info = link_plan_info(plan->p);
    return RV_OK;
}

extern "C" void rv_link_plan_destroy(rv_link_plan* plan) {
    if (!plan) return;
    (void)hipSetDevice(plan->ctx->device);
    link_plan_destroy(plan->p);
    delete plan;
}

extern "C" int rv_link_plan_emit(rv_link_plan* plan, uint64_t first_op, uint64_t n, rv_op* d_ops, rv_link_piece* piece) {
    if (!plan || !piece) return RV_E_ARG;
    const uint64_t n_ops = link_plan_info(plan->p).n_ops;
    if (first_op > n_ops || n > n_ops - first_op || (n && !d_ops)) return RV_E_ARG;
    if (n >= LK_MAX_EMIT) return RV_E_UNSUPPORTED;
    rv_ctx* ctx = plan->ctx;
    return guarded([&]() -> int {
        LibBusy busy_guard;
        HIPCHK(hipSetDevice(ctx->device));
        if (n)
            if (int rb = device_bytes_ok(ctx, d_ops, n * sizeof(rv_op), 8)) return rb;
        const int rc = link_plan_emit(plan->p, first_op, n, d_ops, piece);
        if (rc == RV_E_DEVICE) g_last_error = "device linker: HIP error";
        if (rc == RV_E_NOMEM) g_last_error = "device linker: out of device memory";
        return rc;
    });
}
