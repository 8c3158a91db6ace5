// Part of api.hip (#included there, one translation unit, ahead of compact.inc, prune.inc and fold.inc): the one way a feed reaches
// a windowed stage (rv_compactor_*, rv_pruner_*, rv_folder_*; the stage contract is DESIGN §17.6).

// the error texts of a stage's calls (what: "windowed pruning")
static int stage_code(int rc, const char* what) {
    if (rc == RV_E_DEVICE) g_last_error = std::string(what) + ": HIP error";
    if (rc == RV_E_NOMEM) g_last_error = std::string(what) + ": out of device memory";
    return rc;
}

namespace {
// the uploaded copy of a host feed: given back on every way out, once the stream is idle
struct Upload {
    rv_ctx* ctx;
    void* d = nullptr;
    ~Upload() {
        if (d) {
            (void)hipStreamSynchronize(ctx->stream);
            ctx->release(d);
        }
    }
};

// what a stage says of one of its feeds
struct PassShape {
    const char* what;      // the stage, as the error texts name it
    const char* arg_text;  // the text of an RV_E_ARG from the call itself (nullptr: none)
    bool need_out;         // d_out must be given
    bool in_place;         // d_out == ops (in device memory) is the in-place form; any other overlap is refused either way
    size_t out_records;    // the records d_out has room for
    uint32_t* d_index;     // out_records words beside d_out (the pruner's old_index), or nullptr
};
}  // namespace

// A feed of n_ops records at `ops` (host memory, uploaded here, or device memory) to a stage of `ctx` (nullptr: the handle was).
// admit(): what the stage answers before it looks at the ops -- asked first, and before the upload: a call out of order is RV_E_ARG
// whatever its pointers are, and moves nothing.  Then the pointers, the overlap, the upload, and call(d_ops, upload_bytes).
template <class Admit, class Call>
static int stage_pass(rv_ctx* ctx, const PassShape& s, const rv_op* ops, size_t n_ops, int ops_on_device, rv_op* d_out, Admit&& admit, Call&& call) {
    if (!ctx || (n_ops && (!ops || (s.need_out && !d_out)))) return RV_E_ARG;
    if (n_ops > (size_t)-1 / sizeof(rv_op)) return RV_E_UNSUPPORTED;
    if (s.out_records > (size_t)-1 / sizeof(rv_op)) return RV_E_ARG;
    return guarded([&]() -> int {
        LibBusy busy_guard;
        HIPCHK(hipSetDevice(ctx->device));
        const size_t bytes = n_ops * sizeof(rv_op), out_bytes = s.out_records * sizeof(rv_op);
        if (const int rc = admit()) return rc;
        if (n_ops) {
            if (ops_on_device)
                if (int rb = device_bytes_ok(ctx, ops, bytes, 8)) return rb;
            if (d_out && out_bytes && !(s.in_place && ops_on_device && d_out == ops)) {
                if (int rb = device_bytes_ok(ctx, d_out, out_bytes, 8)) return rb;
                // (a tile's stores would land where another tile's records are still to be read)
                const uint8_t *i0 = (const uint8_t*)ops, *o0 = (const uint8_t*)d_out;
                if (ops_on_device && o0 < i0 + bytes && i0 < o0 + out_bytes) return RV_E_ARG;
                if (s.d_index)
                    if (int rb = device_bytes_ok(ctx, s.d_index, s.out_records * sizeof(uint32_t), 4)) return rb;
            }
        }
        Upload up{ctx};
        const rv_op* d_ops = ops;
        if (n_ops && !ops_on_device) {
            if (ctx->alloc(bytes, &up.d) != RV_OK) return stage_code(RV_E_NOMEM, s.what);
            if (hipMemcpyAsync(up.d, ops, bytes, hipMemcpyHostToDevice, ctx->stream) != hipSuccess) return stage_code(RV_E_DEVICE, s.what);
            d_ops = (const rv_op*)up.d;
        }
        const int rc = call(d_ops, up.d ? bytes : (size_t)0);
        if (rc == RV_E_ARG && s.arg_text) g_last_error = s.arg_text;
        return stage_code(rc, s.what);
    });
}
