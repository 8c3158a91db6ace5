// Part of api.hip (#included there, one translation unit): rv_bristol_parse_device -- the gate-line kernels of bristol_dev.hip on the
// context's stream, the text (when it comes from host memory) and the work memory in the context arena.  The header lines go through
// bristol.cpp's header code, the one rv_bristol_parse runs.

extern "C" int rv_hook_bristol_tiles(uint32_t out[2]) {
    if (!out) return RV_E_ARG;
    out[0] = BRISTOL_TILE_BYTES;
    out[1] = BRISTOL_WG_LINES;
    return RV_OK;
}

namespace {
// arena blocks of one call, given back when it ends (the stream is idle by then: bristol_gates_device synchronises it)
struct ArenaBlocks {
    rv_ctx* ctx;
    std::vector<void*> ps;
    explicit ArenaBlocks(rv_ctx* c) : ctx(c) {}
    void* get(size_t bytes) {
        void* p = nullptr;
        if (ctx->alloc(bytes, &p) != RV_OK) return nullptr;
        ps.push_back(p);
        return p;
    }
    ~ArenaBlocks() {
        (void)hipStreamSynchronize(ctx->stream);
        for (void* p : ps) ctx->release(p);
    }
};

// the first bytes of a device text that hold four non-blank lines (the header lines and the first gate line at most), or all of it
int bristol_device_prefix(rv_ctx* ctx, const char* d_text, size_t len, std::vector<char>& prefix) {
    for (size_t take = std::min<size_t>(len, 4096);; take = std::min<size_t>(len, take * 2)) {
        const size_t have = prefix.size();
        prefix.resize(take);
        if (take > have) {
            HIPCHK(hipMemcpyAsync(prefix.data() + have, d_text + have, take - have, hipMemcpyDeviceToHost, ctx->stream));
            HIPCHK(hipStreamSynchronize(ctx->stream));
        }
        if (take == len) return RV_OK;
        int lines = 0;
        bool token = false;
        for (size_t i = 0; i < take && lines < 4; i++) {
            const char c = prefix[i];
            if (c == '\n') lines += token, token = false;
            else if (c != ' ' && c != '\t' && c != '\r') token = true;
        }
        if (lines >= 4) return RV_OK;
    }
}
}  // namespace

extern "C" int rv_bristol_parse_device(rv_ctx* ctx, const char* text, size_t len, int text_on_device, int format, const uint8_t* expected_outputs,
                                       size_t n_expected, rv_op* d_ops, size_t cap_ops, size_t* n_ops, rv_bristol_info* info) {
    if (!ctx || !text || !n_ops) return RV_E_ARG;
    *n_ops = 0;
    if (d_ops && cap_ops > (size_t)-1 / sizeof(rv_op)) return RV_E_ARG;
    try {
        LibBusy busy_guard;  // (compile.h: the background unmapper keeps still while the GPU is driven)
        HIPCHK(hipSetDevice(ctx->device));
        if (d_ops)
            if (int rb = device_bytes_ok(ctx, d_ops, cap_ops * sizeof(rv_op), 8)) return rb;
        if (text_on_device)
            if (int rb = device_bytes_ok(ctx, text, len, 1)) return rb;
        if (len >= (1ull << 32)) return RV_E_UNSUPPORTED;

        // the header lines, on the host
        rv_bristol_info bi;
        size_t gates_offset = 0;
        int rc;
        if (text_on_device) {
            std::vector<char> prefix;
            if ((rc = bristol_device_prefix(ctx, text, len, prefix))) return rc;
            rc = rv_internal_bristol_header(prefix.data() ? prefix.data() : "", prefix.size(), len, format, expected_outputs != nullptr, n_expected, &bi,
                                            &gates_offset);
        } else {
            rc = rv_internal_bristol_header(text, len, len, format, expected_outputs != nullptr, n_expected, &bi, &gates_offset);
        }
        if (rc) return rc;
        const uint64_t n_pairs = expected_outputs ? bi.n_outputs : 0;
        bi.gf2_wires = bi.n_wires + n_pairs;
        const bool wires_fit = bi.gf2_wires <= 0xFFFFFFFFull;

        // the text and the expected outputs in arena memory (a plain copy from pageable memory: DESIGN §18)
        ArenaBlocks blocks_(ctx);
        const uint8_t* d_text = (const uint8_t*)text;
        if (!text_on_device) {
            void* p = blocks_.get(len);
            if (!p) {
                g_last_error = "device Bristol parser: out of device memory";
                return RV_E_NOMEM;
            }
            if (len) HIPCHK(hipMemcpyAsync(p, text, len, hipMemcpyHostToDevice, ctx->stream));
            d_text = (const uint8_t*)p;
        }
        // (records are written only if they can fit; the expected bits are uploaded only then, so no allocation follows the header's
        // claims: n_pairs bytes are fewer than the caller's own buffer)
        rv_op* out = d_ops && wires_fit && bi.n_inputs + 2 * n_pairs <= cap_ops ? d_ops : nullptr;
        uint8_t* d_exp = nullptr;
        if (out && n_pairs) {
            d_exp = (uint8_t*)blocks_.get(n_pairs);
            if (!d_exp) {
                g_last_error = "device Bristol parser: out of device memory";
                return RV_E_NOMEM;
            }
            HIPCHK(hipMemcpyAsync(d_exp, expected_outputs, n_pairs, hipMemcpyHostToDevice, ctx->stream));
        }
        BristolGates g;
        rc = bristol_gates_device(ctx->stream, ctx_dev_allocator(ctx), d_text, len, gates_offset, bi.n_gates, bi.n_wires, bi.n_inputs, d_exp, n_pairs, out,
                                  cap_ops, &g);
        if (rc == RV_E_DEVICE) g_last_error = "device Bristol parser: HIP error";
        if (rc == RV_E_NOMEM) g_last_error = "device Bristol parser: out of device memory";
        if (rc) return rc;
        if (g.code) return g.code;
        if (!wires_fit) return RV_E_UNSUPPORTED;
        bi.n_and = g.n_and, bi.n_xor = g.n_xor, bi.n_inv = g.n_inv, bi.n_other = g.n_other;
        *n_ops = (size_t)(bi.n_inputs + g.gate_ops + 2 * n_pairs);
        if (info) *info = bi;
        if (!g.written) {
            g_last_error = "rv_bristol_parse_device: d_ops holds fewer records than the text stands for (*n_ops)";
            return RV_E_ARG;
        }
        return RV_OK;
    } catch (...) {
        g_last_error = "out of host memory";
        return RV_E_NOMEM;
    }
}
