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

// ---- a text read in windows (rv_bristol_reader_*): the state machine is bristol_dev.h's (br_window_*), the kernels one buffer's ----
struct rv_bristol_reader {
    rv_ctx* ctx;
    BrWindowState s;
    std::vector<uint8_t> expected;  // the caller's expected outputs, uploaded with the feed that writes the pairs
    void* d_carry = nullptr;        // the unfinished line (arena memory, s.carry bytes)
};

extern "C" int rv_bristol_reader_begin(rv_ctx* ctx, uint64_t file_len, int format, const uint8_t* expected_outputs, size_t n_expected,
                                       rv_bristol_reader** out) {
    if (!ctx || !out) return RV_E_ARG;
    *out = nullptr;
    try {
        std::unique_ptr<rv_bristol_reader> r(new rv_bristol_reader);
        r->ctx = ctx;
        br_window_begin(r->s, file_len, format, expected_outputs != nullptr, n_expected);
        if (expected_outputs) r->expected.assign(expected_outputs, expected_outputs + n_expected);
        *out = r.release();
        return RV_OK;
    } catch (...) {
        g_last_error = "out of host memory";
        return RV_E_NOMEM;
    }
}

extern "C" void rv_bristol_reader_destroy(rv_bristol_reader* r) {
    if (!r) return;
    if (r->d_carry) r->ctx->release(r->d_carry);  // (every feed leaves the stream idle)
    delete r;
}

extern "C" int rv_bristol_reader_header(rv_bristol_reader* r, rv_bristol_info* info) {
    if (!r || !info || r->s.code || !r->s.have_header) return RV_E_ARG;
    *info = r->s.info;
    return RV_OK;
}

extern "C" int rv_bristol_reader_finish(rv_bristol_reader* r, rv_bristol_info* info) {
    if (!r) return RV_E_ARG;
    return br_window_finish(r->s, info);
}

extern "C" int rv_hook_bristol_reader_resume(rv_bristol_reader* r, uint64_t file_off, uint64_t next_line, uint64_t next_op) {
    if (!r || r->s.code || file_off > r->s.file_len) return RV_E_ARG;
    try {
        BrWindowState& s = r->s;
        if (!s.have_header) {  // (the header lines alone were fed: the look at the first gate line is not waited for)
            const BrHeadMark m = br_window_mark(s);
            if (int rc = br_window_header(s)) {
                s.code = 0;
                br_window_rollback(s, m);
                return rc;
            }
        }
        if (next_line > s.info.n_gates) return RV_E_ARG;
        s.head = std::vector<char>();
        s.fed = file_off, s.lines_done = next_line, s.ops_done = next_op;
        s.inputs_out = true, s.pairs_out = false, s.carry = 0;
        if (r->d_carry) r->ctx->release(r->d_carry);
        r->d_carry = nullptr;
        return RV_OK;
    } catch (...) {
        return RV_E_NOMEM;
    }
}

extern "C" int rv_bristol_reader_feed(rv_bristol_reader* r, const char* text, size_t len, int text_on_device, rv_op* d_ops, size_t cap_ops,
                                      rv_bristol_piece* piece) {
    if (!r || !piece) return RV_E_ARG;
    if ((uint64_t)len >= (1ull << 32)) return RV_E_ARG;
    BrWindowState& s = r->s;
    rv_ctx* ctx = r->ctx;
    if (s.code || (!text && len) || len > s.file_len - s.fed) return RV_E_ARG;
    if (d_ops && cap_ops > (size_t)-1 / sizeof(rv_op)) return RV_E_ARG;
    const bool had_header = s.have_header;
    const BrHeadMark mark = br_window_mark(s);
    // (a feed that fails for a reason that is not the text's leaves the reader as it found it)
    auto back = [&](int rc) {
        if (!had_header) br_window_rollback(s, mark);
        return rc;
    };
    try {
        LibBusy busy_guard;
        HIPCHK(hipSetDevice(ctx->device));
        if (d_ops)
            if (int rb = device_bytes_ok(ctx, d_ops, cap_ops * sizeof(rv_op), 8)) return rb;
        if (text_on_device && len)
            if (int rb = device_bytes_ok(ctx, text, len, 1)) return rb;
        if (s.carry + (uint64_t)len >= (1ull << 32)) return RV_E_UNSUPPORTED;
        if (br_window_complete(s)) {  // (bytes behind the last gate line are never judged)
            br_window_skip(s, len, piece);
            return RV_OK;
        }

        // the header, on the host: the first bytes, until they hold four whole non-blank lines or the file ends
        size_t taken = 0, host_len = 0;
        if (!had_header) {
            bool ready = br_window_head_scan(s, s.fed);
            while (!ready) {
                const size_t need = br_window_head_need(s, len - taken);
                if (!need) break;
                const size_t have = s.head.size();
                s.head.resize(have + need);
                if (text_on_device) {
                    if (hipMemcpyAsync(s.head.data() + have, text + taken, need, hipMemcpyDeviceToHost, ctx->stream) != hipSuccess ||
                        hipStreamSynchronize(ctx->stream) != hipSuccess) {
                        g_last_error = "device Bristol reader: HIP error";
                        return back(RV_E_DEVICE);
                    }
                } else {
                    memcpy(s.head.data() + have, text + taken, need);
                }
                taken += need;
                ready = br_window_head_scan(s, s.fed + taken);
            }
            if (!ready) {
                br_window_skip(s, len, piece);
                return RV_OK;
            }
            if (int rc = br_window_header(s)) return rc;
            host_len = s.head.size() - s.gates_offset;
        }
        const uint64_t bytes = s.carry + host_len + (len - taken);
        if (bytes >= (1ull << 32)) return back(RV_E_UNSUPPORTED);
        const BrWindowLaunch l = br_window_launch(s, len);

        // the buffer: carry, header bytes behind the last header line, the window (a device window is copied, too: DESIGN §18.6)
        ArenaBlocks blocks_(ctx);
        uint8_t* d_buf = (uint8_t*)blocks_.get(std::max<size_t>((size_t)bytes, 16));
        const bool may_finish = br_line_cap(bytes, l.want) == l.want;  // (else a line is missing or one is bad: no pairs)
        uint8_t* d_exp = nullptr;
        if (d_ops && l.n_pairs && may_finish) d_exp = (uint8_t*)blocks_.get(l.n_pairs);
        if (!d_buf || (d_ops && l.n_pairs && may_finish && !d_exp)) {
            g_last_error = "device Bristol reader: out of device memory";
            return back(RV_E_NOMEM);
        }
        hipError_t e = hipSuccess;
        if (s.carry) e = hipMemcpyAsync(d_buf, r->d_carry, s.carry, hipMemcpyDeviceToDevice, ctx->stream);
        if (e == hipSuccess && host_len) e = hipMemcpyAsync(d_buf + s.carry, s.head.data() + s.gates_offset, host_len, hipMemcpyHostToDevice, ctx->stream);
        if (e == hipSuccess && len > taken)
            e = hipMemcpyAsync(d_buf + s.carry + host_len, text + taken, len - taken, text_on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice,
                               ctx->stream);
        if (e == hipSuccess && d_exp) e = hipMemcpyAsync(d_exp, r->expected.data(), l.n_pairs, hipMemcpyHostToDevice, ctx->stream);
        if (e != hipSuccess) {
            g_last_error = "device Bristol reader: HIP error";
            return back(RV_E_DEVICE);
        }
        BrWindowLaunch lk = l;
        if (!may_finish) lk.n_pairs = 0;
        BrWindowResult res;
        int rc = bristol_window_device(ctx->stream, ctx_dev_allocator(ctx), d_buf, (size_t)bytes, lk, s.info.n_wires, d_exp, d_ops, cap_ops, &res);
        if (rc == RV_E_DEVICE) g_last_error = "device Bristol reader: HIP error";
        if (rc == RV_E_NOMEM) g_last_error = "device Bristol reader: out of device memory";
        if (rc) return back(rc);

        // the new carry's block first, so that the state moves only when nothing can fail any more
        const uint64_t carry_bytes = res.code ? 0 : br_window_carry(l, res, bytes);
        void* d_new = nullptr;
        if (carry_bytes && ctx->alloc((size_t)carry_bytes, &d_new) != RV_OK) {
            g_last_error = "device Bristol reader: out of device memory";
            return back(RV_E_NOMEM);
        }
        rc = br_window_done(s, len, bytes, l, res, d_ops == nullptr, cap_ops, piece);
        if (rc) {
            if (d_new) ctx->release(d_new);
            if (rc == RV_E_ARG && !s.code) {
                g_last_error = "rv_bristol_reader_feed: d_ops holds fewer records than this feed delivers (piece->n_ops)";
                return back(rc);
            }
            return rc;
        }
        if (carry_bytes) {
            HIPCHK(hipMemcpyAsync(d_new, d_buf + res.carry_from, carry_bytes, hipMemcpyDeviceToDevice, ctx->stream));
            HIPCHK(hipStreamSynchronize(ctx->stream));
        }
        if (r->d_carry) ctx->release(r->d_carry);
        r->d_carry = d_new;
        s.head = std::vector<char>();
        return RV_OK;
    } catch (...) {
        g_last_error = "out of host memory";
        return back(RV_E_NOMEM);
    }
}
