// Part of api.hip (#included there, one translation unit, behind bristol.inc): rv_witness_parse_device, rv_witness_reader_* and
// rv_witness_write_device -- the kernels of witness_dev.hip on the context's stream, the text (when it comes from host memory), the
// marks and the work memory in the context arena.

extern "C" int rv_hook_witness_text_tiles(uint32_t out[2]) {
    if (!out) return RV_E_ARG;
    out[0] = WT_TILE_BYTES * WT_WG_TILES;
    out[1] = WT_WRITE_TILE_BYTES;
    return RV_OK;
}

namespace {
bool ranges_meet(const void* a, size_t na, const void* b, size_t nb) {
    const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
    return na && nb && x < y + nb && y < x + na;
}

// what rv_witness_parse_device and a reader's feed share; marks: validated by the caller
int witness_parse_impl(rv_ctx* ctx, const char* text, size_t len, int text_on_device, uint8_t* d_bits, size_t cap, size_t* n_bits, const uint64_t* marks,
                       size_t n_marks, uint64_t* bits_before, const char* who) {
    LibBusy busy_guard;  // (compile.h: the background unmapper keeps still while the GPU is driven)
    HIPCHK(hipSetDevice(ctx->device));
    if (d_bits)
        if (int rb = device_bytes_ok(ctx, d_bits, cap, 1)) return rb;
    if (text_on_device && len)
        if (int rb = device_bytes_ok(ctx, text, len, 1)) return rb;
    if (len >= (1ull << 32)) return RV_E_UNSUPPORTED;
    if (text_on_device && d_bits && ranges_meet(text, len, d_bits, cap)) return RV_E_ARG;

    // the text and the marks in arena memory (a plain copy from pageable memory, as the Bristol parser's)
    ArenaBlocks blocks_(ctx);
    const uint8_t* d_text = (const uint8_t*)text;
    if (!text_on_device && len) {
        void* p = blocks_.get(len);
        if (!p) {
            g_last_error = "device witness parser: out of device memory";
            return RV_E_NOMEM;
        }
        HIPCHK(hipMemcpyAsync(p, text, len, hipMemcpyHostToDevice, ctx->stream));
        g_wit_traffic[0].fetch_add(len, std::memory_order_relaxed);  // (the witness, in its text form)
        d_text = (const uint8_t*)p;
    }
    uint64_t* d_marks = nullptr;
    if (n_marks && len) {
        d_marks = (uint64_t*)blocks_.get(n_marks * sizeof(uint64_t));
        if (!d_marks) {
            g_last_error = "device witness parser: out of device memory";
            return RV_E_NOMEM;
        }
        HIPCHK(hipMemcpyAsync(d_marks, marks, n_marks * sizeof(uint64_t), hipMemcpyHostToDevice, ctx->stream));
    }
    WitnessParse r;
    const int rc = witness_parse_device(ctx->stream, ctx_dev_allocator(ctx), d_text, len, d_bits, d_bits ? cap : 0, d_marks, n_marks, bits_before, &r);
    if (rc == RV_E_DEVICE) g_last_error = "device witness parser: HIP error";
    if (rc == RV_E_NOMEM) g_last_error = "device witness parser: out of device memory";
    if (rc) return rc;
    *n_bits = (size_t)r.bits;
    if (d_bits && !r.written) {
        g_last_error = std::string(who) + ": d_bits holds fewer bytes than the text has bits (*n_bits)";
        return RV_E_ARG;
    }
    return RV_OK;
}
}  // namespace

extern "C" int rv_witness_parse_device(rv_ctx* ctx, const char* text, size_t len, int text_on_device, uint8_t* d_bits, size_t cap, size_t* n_bits,
                                       const uint64_t* marks, size_t n_marks, uint64_t* bits_before) {
    if (!ctx || !n_bits || (!text && len) || (n_marks && (!marks || !bits_before))) return RV_E_ARG;
    *n_bits = 0;
    if (n_marks > (size_t)-1 / sizeof(uint64_t)) return RV_E_ARG;
    for (size_t m = 0; m < n_marks; m++)
        if (marks[m] > len || (m && marks[m] < marks[m - 1])) return RV_E_ARG;
    return guarded([&] { return witness_parse_impl(ctx, text, len, text_on_device, d_bits, cap, n_bits, marks, n_marks, bits_before, "rv_witness_parse_device"); });
}

// ---- a text read in windows: nothing is carried between feeds but the two totals ----
struct rv_witness_reader {
    rv_ctx* ctx;
    uint64_t bytes_fed, bits_total;
};

extern "C" int rv_witness_reader_begin(rv_ctx* ctx, rv_witness_reader** out) {
    if (!ctx || !out) return RV_E_ARG;
    *out = new (std::nothrow) rv_witness_reader{ctx, 0, 0};
    return *out ? RV_OK : RV_E_NOMEM;
}

extern "C" void rv_witness_reader_destroy(rv_witness_reader* r) { delete r; }

extern "C" int rv_witness_reader_feed(rv_witness_reader* r, const char* text, size_t len, int text_on_device, uint8_t* d_bits, size_t cap, size_t* n_bits) {
    if (!r || !n_bits || (!text && len)) return RV_E_ARG;
    *n_bits = 0;
    const int rc =
        guarded([&] { return witness_parse_impl(r->ctx, text, len, text_on_device, d_bits, cap, n_bits, nullptr, 0, nullptr, "rv_witness_reader_feed"); });
    if (rc == RV_OK) r->bytes_fed += len, r->bits_total += *n_bits;  // (any other answer leaves the reader as it was)
    return rc;
}

extern "C" int rv_witness_reader_finish(rv_witness_reader* r, uint64_t* bytes_fed, uint64_t* bits_total) {
    if (!r) return RV_E_ARG;
    if (bytes_fed) *bytes_fed = r->bytes_fed;
    if (bits_total) *bits_total = r->bits_total;
    return RV_OK;
}

extern "C" int rv_witness_write_device(rv_ctx* ctx, const uint8_t* d_bits, size_t n, uint64_t line_bits, char* d_text, size_t cap, size_t* len) {
    if (!ctx || !len || (!d_bits && n)) return RV_E_ARG;
    *len = 0;
    return guarded([&]() -> int {
        LibBusy busy_guard;
        HIPCHK(hipSetDevice(ctx->device));
        if (n)
            if (int rb = device_bytes_ok(ctx, d_bits, n, 1)) return rb;
        if (d_text)
            if (int rb = device_bytes_ok(ctx, d_text, cap, 1)) return rb;
        const uint64_t need = wt_text_len(n, line_bits);
        if ((uint64_t)n >= (1ull << 32) || need >= (1ull << 32)) return RV_E_UNSUPPORTED;
        *len = (size_t)need;
        if (!d_text) return RV_OK;
        if (cap < need) {
            g_last_error = "rv_witness_write_device: d_text is shorter than the text (*len)";
            return RV_E_ARG;
        }
        if (ranges_meet(d_bits, n, d_text, (size_t)need)) return RV_E_ARG;
        bool bad = false;
        const int rc = witness_write_device(ctx->stream, ctx_dev_allocator(ctx), d_bits, n, line_bits, (uint8_t*)d_text, &bad);
        if (rc == RV_E_DEVICE) g_last_error = "device witness writer: HIP error";
        if (rc == RV_E_NOMEM) g_last_error = "device witness writer: out of device memory";
        if (rc) return rc;
        return bad ? RV_E_ARG : RV_OK;
    });
}
