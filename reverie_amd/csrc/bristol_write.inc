// Part of api.hip (#included there, one translation unit, behind bincode.inc): rv_bristol_write_device, and the two writers that are
// fed in windows, rv_bristol_writer_* and rv_program_writer_* -- the kernels of bristol_write.hip and the write kernels of
// bincode_dev.hip on the context's stream, the ops (when they come from host memory) and the work memory in the context arena.

extern "C" int rv_hook_bristol_write_tiles(uint32_t out[2]) {
    if (!out) return RV_E_ARG;
    out[0] = BRISTOL_WRITE_TILE;
    out[1] = BRISTOL_WRITE_SCAN_BLOCK;
    return RV_OK;
}

extern "C" int rv_bristol_write_device(rv_ctx* ctx, const rv_op* d_ops, size_t n_ops, uint64_t n_wires, uint64_t n_outputs, char* d_text, size_t cap,
                                       size_t* len) {
    if (!ctx || (!d_ops && n_ops) || !len) return RV_E_ARG;
    *len = 0;
    if (n_ops > (size_t)-1 / sizeof(rv_op)) return RV_E_ARG;
    try {
        LibBusy busy_guard;
        HIPCHK(hipSetDevice(ctx->device));
        if (n_ops)
            if (int rb = device_bytes_ok(ctx, d_ops, n_ops * sizeof(rv_op), 8)) return rb;
        if (d_text)
            if (int rb = device_bytes_ok(ctx, d_text, cap, 1)) return rb;
        // (a list this long holds an Input whose position no 32-bit dst can name, or 2^32 bytes of lines)
        if ((uint64_t)n_ops >= (1ull << 32)) return RV_E_UNSUPPORTED;
        BwJob job = {};
        job.total_ops = n_ops, job.n_wires = n_wires, job.n_outputs = n_outputs, job.whole = 1, job.header = 1;
        BristolWrite w;
        const int rc = bristol_write_device(ctx->stream, ctx_dev_allocator(ctx), d_ops, n_ops, job, (uint8_t*)d_text, d_text ? cap : 0, &w);
        if (rc == RV_E_DEVICE) g_last_error = "device Bristol writer: HIP error";
        if (rc == RV_E_NOMEM) g_last_error = "device Bristol writer: out of device memory";
        if (rc) return rc;
        if (w.code) {
            if (w.record) g_last_error = "rv_bristol_write_device: op " + std::to_string(w.err_op) + " cannot be written as Bristol text";
            return w.code;
        }
        if (w.bytes >= (1ull << 32)) return RV_E_UNSUPPORTED;
        *len = (size_t)w.bytes;
        if (!w.written) {
            g_last_error = "rv_bristol_write_device: d_text is shorter than the text (*len)";
            return RV_E_ARG;
        }
        return RV_OK;
    } catch (...) {
        g_last_error = "out of host memory";
        return RV_E_NOMEM;
    }
}

// ---- writers fed in windows: nothing is carried between feeds but the next ordinal, the file offset and "the header is out" ----
namespace {
struct WriterState {
    rv_ctx* ctx;
    uint64_t n_ops, next_op, file_off;
    bool header_out;
    int code;  // the first code of the records: only destroy is accepted
};
// what a feed checks before anything is launched -> RV_OK, RV_E_ARG or RV_E_UNSUPPORTED; d_ops: the feed's records in device memory
// (uploaded into `up` where they come from the host)
int writer_admit(WriterState& s, const rv_op* ops, size_t n, int ops_on_device, const void* d_out, size_t cap, size_t max_n, ArenaBlocks& up,
                 const rv_op** d_ops) {
    rv_ctx* ctx = s.ctx;
    if (s.code || (!ops && n) || n > s.n_ops - s.next_op) return RV_E_ARG;
    if (n > max_n) return RV_E_UNSUPPORTED;
    HIPCHK(hipSetDevice(ctx->device));
    if (n && ops_on_device)
        if (int rb = device_bytes_ok(ctx, ops, n * sizeof(rv_op), 8)) return rb;
    if (d_out)
        if (int rb = device_bytes_ok(ctx, d_out, cap, 1)) return rb;
    *d_ops = ops;
    if (n && !ops_on_device) {
        void* p = up.get(n * sizeof(rv_op));
        if (!p) {
            g_last_error = "windowed writer: out of device memory";
            return RV_E_NOMEM;
        }
        HIPCHK(hipMemcpyAsync(p, ops, n * sizeof(rv_op), hipMemcpyHostToDevice, ctx->stream));
        *d_ops = (const rv_op*)p;
    }
    return RV_OK;
}
// the feed's answer once the kernels have judged and (where they could) written `bytes` bytes
int writer_done(WriterState& s, size_t n, uint64_t bytes, bool written, rv_writer_piece* piece, const char* who) {
    if (bytes >= (1ull << 32)) return RV_E_UNSUPPORTED;
    *piece = rv_writer_piece{s.next_op, n, s.file_off, bytes};
    if (!written) {
        g_last_error = std::string(who) + ": the buffer is shorter than the feed's bytes (piece->bytes)";
        return RV_E_ARG;
    }
    s.next_op += n, s.file_off += bytes, s.header_out = true;
    return RV_OK;
}
}  // namespace

struct rv_bristol_writer {
    WriterState s;
    uint64_t n_inputs, n_wires, n_outputs;
};

extern "C" int rv_bristol_writer_begin(rv_ctx* ctx, uint64_t n_ops, uint64_t n_inputs, uint64_t n_wires, uint64_t n_outputs, rv_bristol_writer** out) {
    if (!ctx || !out) return RV_E_ARG;
    *out = nullptr;
    if (n_inputs > n_ops || (!n_wires && n_ops)) return RV_E_ARG;
    if (bw_header_code(n_wires, n_inputs, n_outputs)) return RV_E_WIRE_OOB;
    rv_bristol_writer* w = new (std::nothrow) rv_bristol_writer{};
    if (!w) return RV_E_NOMEM;
    w->s.ctx = ctx, w->s.n_ops = n_ops;
    w->n_inputs = n_inputs, w->n_wires = n_wires, w->n_outputs = n_outputs;
    *out = w;
    return RV_OK;
}

extern "C" void rv_bristol_writer_destroy(rv_bristol_writer* w) { delete w; }

extern "C" int rv_bristol_writer_finish(rv_bristol_writer* w) {
    return w && !w->s.code && w->s.header_out && w->s.next_op == w->s.n_ops ? RV_OK : RV_E_ARG;
}

extern "C" int rv_bristol_writer_feed(rv_bristol_writer* w, const rv_op* ops, size_t n, int ops_on_device, char* d_text, size_t cap,
                                      rv_writer_piece* piece) {
    if (!w || !piece) return RV_E_ARG;
    WriterState& s = w->s;
    try {
        LibBusy busy_guard;
        ArenaBlocks up(s.ctx);
        const rv_op* d_ops = nullptr;
        if (int rc = writer_admit(s, ops, n, ops_on_device, d_text, cap, (1ull << 32) - 1, up, &d_ops)) return rc;
        BwJob job = {};
        job.first_op = s.next_op, job.total_ops = s.n_ops, job.n_inputs = w->n_inputs, job.n_wires = w->n_wires, job.n_outputs = w->n_outputs;
        job.header = s.header_out ? 0 : 1;
        BristolWrite r;
        const int rc = bristol_write_device(s.ctx->stream, ctx_dev_allocator(s.ctx), d_ops, n, job, (uint8_t*)d_text, d_text ? cap : 0, &r);
        if (rc == RV_E_DEVICE) g_last_error = "device Bristol writer: HIP error";
        if (rc == RV_E_NOMEM) g_last_error = "device Bristol writer: out of device memory";
        if (rc) return rc;
        if (r.code) {
            g_last_error = "rv_bristol_writer_feed: op " + std::to_string(r.err_op) + " cannot be written as Bristol text";
            return s.code = r.code;
        }
        return writer_done(s, n, r.bytes, r.written, piece, "rv_bristol_writer_feed");
    } catch (...) {
        g_last_error = "out of host memory";
        return RV_E_NOMEM;
    }
}

struct rv_program_writer {
    WriterState s;
};

extern "C" int rv_program_writer_begin(rv_ctx* ctx, uint64_t n_ops, rv_program_writer** out) {
    if (!ctx || !out) return RV_E_ARG;
    *out = nullptr;
    rv_program_writer* w = new (std::nothrow) rv_program_writer{};
    if (!w) return RV_E_NOMEM;
    w->s.ctx = ctx, w->s.n_ops = n_ops;
    *out = w;
    return RV_OK;
}

extern "C" void rv_program_writer_destroy(rv_program_writer* w) { delete w; }

extern "C" int rv_program_writer_finish(rv_program_writer* w) {
    return w && !w->s.code && w->s.header_out && w->s.next_op == w->s.n_ops ? RV_OK : RV_E_ARG;
}

extern "C" int rv_program_writer_feed(rv_program_writer* w, const rv_op* ops, size_t n, int ops_on_device, uint8_t* d_out, size_t cap,
                                      rv_writer_piece* piece) {
    if (!w || !piece) return RV_E_ARG;
    WriterState& s = w->s;
    try {
        LibBusy busy_guard;
        ArenaBlocks up(s.ctx);
        const rv_op* d_ops = nullptr;
        // (the shortest record takes BC_MIN_RECORD bytes: a longer feed cannot stay below 2^32 bytes, whatever it holds)
        if (int rc = writer_admit(s, ops, n, ops_on_device, d_out, cap, ((1ull << 32) - 1 - BC_HEADER_BYTES) / BC_MIN_RECORD, up, &d_ops)) return rc;
        BincodeWrite r;
        const int rc = bincode_write_device(s.ctx->stream, ctx_dev_allocator(s.ctx), d_ops, n, d_out, d_out ? cap : 0, s.header_out ? nullptr : &s.n_ops, &r);
        if (rc == RV_E_DEVICE) g_last_error = "device bincode writer: HIP error";
        if (rc == RV_E_NOMEM) g_last_error = "device bincode writer: out of device memory";
        if (rc) return rc;
        if (r.code) return s.code = r.code;
        return writer_done(s, n, r.bytes, r.written, piece, "rv_program_writer_feed");
    } catch (...) {
        g_last_error = "out of host memory";
        return RV_E_NOMEM;
    }
}
