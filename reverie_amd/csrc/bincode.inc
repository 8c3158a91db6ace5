// Part of api.hip (#included there, one translation unit, behind bristol.inc): rv_program_from_bincode_device and
// rv_program_to_bincode_device -- the kernels of bincode_dev.hip on the context's stream, the file (when it comes from host memory)
// and the work memory in the context arena.

extern "C" int rv_hook_bincode_tiles(uint32_t out[2]) {
    if (!out) return RV_E_ARG;
    out[0] = BINCODE_TILE_BYTES;  // (counted from data[0], not from an aligned address)
    out[1] = BINCODE_SCAN_TILES;
    return RV_OK;
}

extern "C" int rv_program_from_bincode_device(rv_ctx* ctx, const uint8_t* data, size_t len, int data_on_device, rv_op* d_ops, size_t cap_ops,
                                              size_t* n_ops, rv_program_info* info) {
    if (!ctx || !data || !n_ops) return RV_E_ARG;
    *n_ops = 0;
    if (d_ops && cap_ops > (size_t)-1 / sizeof(rv_op)) return RV_E_ARG;
    try {
        LibBusy busy_guard;  // (compile.h: the background unmapper keeps still while the GPU is driven)
        HIPCHK(hipSetDevice(ctx->device));
        if (d_ops)
            if (int rb = device_bytes_ok(ctx, d_ops, cap_ops * sizeof(rv_op), 8)) return rb;
        if (data_on_device)
            if (int rb = device_bytes_ok(ctx, data, len, 1)) return rb;
        if (len >= (1ull << 32)) return RV_E_UNSUPPORTED;

        // the header, on the host: nothing is allocated or launched by what the count claims
        if (len < BC_HEADER_BYTES) return RV_E_BAD_OP;
        uint8_t head[BC_HEADER_BYTES];
        if (data_on_device) {
            HIPCHK(hipMemcpyAsync(head, data, sizeof head, hipMemcpyDeviceToHost, ctx->stream));
            HIPCHK(hipStreamSynchronize(ctx->stream));
        } else {
            memcpy(head, data, sizeof head);
        }
        uint64_t count = 0;
        for (uint32_t k = 0; k < BC_HEADER_BYTES; k++) count |= (uint64_t)head[k] << (8 * k);
        if (count > (len - BC_HEADER_BYTES) / BC_MIN_RECORD) return RV_E_BAD_OP;
        rv_program_info pi = {};
        pi.bytes = BC_HEADER_BYTES;
        if (count == 0) {  // (nothing to read, nothing to write: no capacity is asked for)
            if (info) *info = pi;
            return RV_OK;
        }

        ArenaBlocks blocks_(ctx);
        const uint8_t* d_data = data;
        if (!data_on_device) {
            void* p = blocks_.get(len);
            if (!p) {
                g_last_error = "device bincode reader: out of device memory";
                return RV_E_NOMEM;
            }
            HIPCHK(hipMemcpyAsync(p, data, len, hipMemcpyHostToDevice, ctx->stream));
            d_data = (const uint8_t*)p;
        }
        BincodeRead r;
        const int rc = bincode_read_device(ctx->stream, ctx_dev_allocator(ctx), d_data, len, count, d_ops && count <= cap_ops ? d_ops : nullptr, &r);
        if (rc == RV_E_DEVICE) g_last_error = "device bincode reader: HIP error";
        if (rc == RV_E_NOMEM) g_last_error = "device bincode reader: out of device memory";
        if (rc) return rc;
        if (r.code) return r.code;
        *n_ops = (size_t)count;
        if (info) *info = r.info;
        if (!r.written) {
            g_last_error = "rv_program_from_bincode_device: d_ops holds fewer records than the file (*n_ops)";
            return RV_E_ARG;
        }
        return RV_OK;
    } catch (...) {
        g_last_error = "out of host memory";
        return RV_E_NOMEM;
    }
}

extern "C" int rv_program_to_bincode_device(rv_ctx* ctx, const rv_op* d_ops, size_t n_ops, uint8_t* d_out, size_t cap, size_t* len) {
    if (!ctx || (!d_ops && n_ops) || !len) return RV_E_ARG;
    *len = 0;
    if (n_ops > (size_t)-1 / sizeof(rv_op)) return RV_E_ARG;
    try {
        LibBusy busy_guard;
        HIPCHK(hipSetDevice(ctx->device));
        if (n_ops)
            if (int rb = device_bytes_ok(ctx, d_ops, n_ops * sizeof(rv_op), 8)) return rb;
        if (d_out)
            if (int rb = device_bytes_ok(ctx, d_out, cap, 1)) return rb;
        // (the shortest record takes BC_MIN_RECORD bytes: such a list cannot make a file below 2^32 bytes, whatever it holds)
        if (n_ops > ((1ull << 32) - 1 - BC_HEADER_BYTES) / BC_MIN_RECORD) return RV_E_UNSUPPORTED;
        BincodeWrite w;
        const uint64_t count = n_ops;
        const int rc = bincode_write_device(ctx->stream, ctx_dev_allocator(ctx), d_ops, n_ops, d_out, d_out ? cap : 0, &count, &w);
        if (rc == RV_E_DEVICE) g_last_error = "device bincode writer: HIP error";
        if (rc == RV_E_NOMEM) g_last_error = "device bincode writer: out of device memory";
        if (rc) return rc;
        if (w.code) return w.code;
        if (w.bytes >= (1ull << 32)) return RV_E_UNSUPPORTED;
        *len = (size_t)w.bytes;
        if (!w.written) {
            g_last_error = "rv_program_to_bincode_device: d_out is shorter than the file (*len)";
            return RV_E_ARG;
        }
        return RV_OK;
    } catch (...) {
        g_last_error = "out of host memory";
        return RV_E_NOMEM;
    }
}

// ---- a file read in windows (rv_program_reader_*): the state machine is bincode_dev.h's (bc_window_*), the kernels one window's ----
struct rv_program_reader {
    rv_ctx* ctx;
    BcWindowState s;
};

extern "C" int rv_program_reader_begin(rv_ctx* ctx, uint64_t file_len, rv_program_reader** out) {
    if (!ctx || !out) return RV_E_ARG;
    *out = nullptr;
    rv_program_reader* r = new (std::nothrow) rv_program_reader;
    if (!r) return RV_E_NOMEM;
    r->ctx = ctx;
    bc_window_begin(r->s, file_len);
    *out = r;
    return RV_OK;
}

extern "C" void rv_program_reader_destroy(rv_program_reader* r) { delete r; }

extern "C" int rv_hook_program_reader_resume(rv_program_reader* r, uint64_t file_off, uint64_t next_op) {
    if (!r || file_off > r->s.file_len) return RV_E_ARG;
    bc_window_resume(r->s, file_off, next_op);
    return RV_OK;
}

extern "C" int rv_program_reader_finish(rv_program_reader* r, rv_program_info* info) {
    if (!r) return RV_E_ARG;
    return bc_window_finish(r->s, info);
}

extern "C" int rv_program_reader_feed(rv_program_reader* r, const uint8_t* data, size_t len, int data_on_device, rv_op* d_ops, size_t cap_ops,
                                      rv_program_piece* piece) {
    if (!r || !piece) return RV_E_ARG;
    if ((uint64_t)len >= (1ull << 32)) return RV_E_ARG;
    BcWindowState& s = r->s;
    rv_ctx* ctx = r->ctx;
    if (s.code || (!data && len) || len > s.file_len - s.file_off) return RV_E_ARG;
    if (d_ops && cap_ops < len / BC_MIN_RECORD + 1) {
        g_last_error = "rv_program_reader_feed: d_ops needs room for len / 16 + 1 records";
        return RV_E_ARG;
    }
    try {
        LibBusy busy_guard;
        HIPCHK(hipSetDevice(ctx->device));
        if (d_ops)
            if (int rb = device_bytes_ok(ctx, d_ops, (len / BC_MIN_RECORD + 1) * sizeof(rv_op), 8)) return rb;
        if (data_on_device && len)
            if (int rb = device_bytes_ok(ctx, data, len, 1)) return rb;

        // the header, on the host: nothing is allocated or launched by what the count claims
        uint32_t head_taken = 0;
        if (!s.have_count) {
            uint8_t head[BC_HEADER_BYTES];
            head_taken = bc_window_head_need(s, len);
            if (head_taken && data_on_device) {
                HIPCHK(hipMemcpyAsync(head, data, head_taken, hipMemcpyDeviceToHost, ctx->stream));
                HIPCHK(hipStreamSynchronize(ctx->stream));
            } else if (head_taken) {
                memcpy(head, data, head_taken);
            }
            if (int code = bc_window_head(s, head, head_taken, len)) return code;
            if (!s.have_count) {
                *piece = rv_program_piece{};
                return RV_OK;
            }
        }
        if (s.done || !len) {
            bc_window_skip(s, len, piece);
            return RV_OK;
        }

        ArenaBlocks blocks_(ctx);
        const uint8_t* d_data = data;
        if (!data_on_device) {
            void* p = blocks_.get(len);
            if (!p) {
                g_last_error = "device bincode reader: out of device memory";
                return RV_E_NOMEM;
            }
            HIPCHK(hipMemcpyAsync(p, data, len, hipMemcpyHostToDevice, ctx->stream));
            d_data = (const uint8_t*)p;
        }
        BcWindowResult res;
        const int rc = bincode_window_device(ctx->stream, ctx_dev_allocator(ctx), d_data, len, bc_window_launch(s, head_taken), s.carry, d_ops, &res);
        if (rc == RV_E_DEVICE) g_last_error = "device bincode reader: HIP error";
        if (rc == RV_E_NOMEM) g_last_error = "device bincode reader: out of device memory";
        if (rc) return rc;
        return bc_window_done(s, len, res, piece);
    } catch (...) {
        g_last_error = "out of host memory";
        return RV_E_NOMEM;
    }
}
