// rv_evaluate / rv_evaluate_batch: cleartext evaluation of a compiled circuit on a batch of witnesses (kernels: eval.hip).
// Included by api.hip.  rv_evaluate_batch_device (witness_dev.inc) runs the same body with the witnesses read in device memory
// (WitSrc) and the results written there (EvalDst).

// The schedule the evaluations ran: [0] one launch per level, [1] one walking workgroup per slice of witness words (rv_hook_eval_schedules)
static std::atomic<uint64_t> g_eval_sched[2];

// RV_COMPILE_KEEP_WIRES: the final wire forms to HBM (rv_circuit_compile_impl; c is destroyed by the caller on failure)
static int eval_upload_wires(rv_ctx* ctx, rv_circuit* c) {
    const Compiled& cc = c->cc;
    c->keep_wires = true;
    if (!cc.wire_forms.empty()) {
        if (int rc = dalloc(ctx, cc.wire_forms.size(), &c->d_wire_forms)) return rc;
        HIPCHK(hipMemcpyAsync(c->d_wire_forms, cc.wire_forms.data(), cc.wire_forms.size() * sizeof(WireForm), hipMemcpyHostToDevice, ctx->stream));
    }
    if (!cc.wire_ssa64.empty()) {
        if (int rc = dalloc(ctx, cc.wire_ssa64.size(), &c->d_wire_ssa64)) return rc;
        HIPCHK(hipMemcpyAsync(c->d_wire_ssa64, cc.wire_ssa64.data(), cc.wire_ssa64.size() * 4, hipMemcpyHostToDevice, ctx->stream));
    }
    HIPCHK(hipStreamSynchronize(ctx->stream));
    return RV_OK;
}

// Which schedule runs a circuit (DESIGN.md §13).  A level of a deep, narrow circuit (SHA-256, AES) is a few dozen gates: launched on
// its own it costs the launch floor, so one workgroup per slice of witness words walks all levels instead, __syncthreads() between
// them.  Wide levels (the 10^7-gate benchmark circuit: ~55 000 gates each) need the whole GPU: one launch per level.  The measure is
// the work of an average level for one witness word: GF(2) gates plus 32 x Z64 gates (a Z64 gate takes a thread per witness).
static bool eval_walks(const Compiled& cc) {
    const uint64_t n_levels = cc.level_range.size();
    if (n_levels < 2) return false;
    return (cc.gates.size() + 32 * (uint64_t)cc.gates64.size()) / n_levels <= 2048;
}

// The gate levels of a compiled circuit (eval_part) or streaming chunk (eval_stream.inc) on the values of p, by the schedule
// eval_walks chooses (counted in g_eval_sched).  d_ls64: the Z64 level table on the device -- needed when the circuit walks
// and has Z64 gates, else unread.
static void eval_run_levels(hipStream_t s, const EvalParams& p, const Compiled& cc, const Gate* d_gates, const LevelRange* d_lr,
                            const Gate64* d_gates64, const uint32_t* d_ls64) {
    const uint32_t n_levels = (uint32_t)cc.level_range.size();
    if (eval_walks(cc)) {
        // a slice of one witness word per workgroup (up to 256 workgroups; more words: wider slices)
        const uint32_t S = (uint32_t)((p.W + 255) / 256);
        const uint64_t per_level = (cc.gates.size() + 32 * (uint64_t)cc.gates64.size()) / n_levels * S;
        launch_eval_walk(s, p, d_gates, d_lr, d_gates64, cc.gates64.empty() ? nullptr : d_ls64, n_levels, S, per_level <= 256 ? 256 : 1024);
        g_eval_sched[1]++;
    } else {
        for (uint32_t l = 0; l < n_levels; l++) {
            const LevelRange& r = cc.level_range[l];
            const uint32_t lo64 = cc.gates64.empty() ? 0 : cc.level_start64[l], hi64 = cc.gates64.empty() ? 0 : cc.level_start64[l + 1];
            launch_eval_level(s, p, d_gates, r.lo, r.hi - r.lo, d_gates64, lo64, hi64 - lo64);
        }
        g_eval_sched[0]++;
    }
}

// the op-list index of the AssertZero with reconstruction ordinal x (UINT64_MAX for none)
static uint64_t eval_assert_op(const std::vector<uint32_t>& rec, const std::vector<uint64_t>& op, uint32_t x) {
    if (x == UINT32_MAX) return UINT64_MAX;
    const auto it = std::lower_bound(rec.begin(), rec.end(), x);
    return (it != rec.end() && *it == x) ? op[(size_t)(it - rec.begin())] : UINT64_MAX;
}

// Where an evaluation's results go.  rv_evaluate_batch: host arrays, every wire's value per witness (n2 / n64 = the wire counts).
// rv_evaluate_batch_device (dev): the caller's device buffers, n2 / n64 selected wires per witness -- d_sel2 / d_sel64: their indices
// on the device, null = every wire in order -- and no result byte goes to the host.  A null values pointer: that domain is not wanted.
struct EvalDst {
    uint8_t* gf2_values;
    uint64_t* z64_values;
    rv_eval_status* st;
    size_t n2, n64;
    bool dev;
    const uint32_t *d_sel2, *d_sel64;
    EvalDst from(size_t b) const {  // witnesses b, b + 1, ...
        EvalDst o = *this;
        if (gf2_values) o.gf2_values += b * n2;
        if (z64_values) o.z64_values += b * n64;
        o.st += b;
        return o;
    }
};

// rv_evaluate_batch_device: the circuit's ordinal -> op index tables on the device, uploaded once per circuit (k_eval_status)
static int eval_assert_tables(rv_ctx* ctx, const rv_circuit* c, EvalFold* f) {
    const Compiled& cc = c->cc;
    std::lock_guard<std::mutex> lk(c->eval_mu);
    if (!c->assert_tables_up) {
        hipStream_t s = ctx->stream;
        auto up = [&](const auto& v, auto** d) -> int {
            if (v.empty()) return RV_OK;
            if (int rc = dalloc(ctx, v.size(), d)) return rc;
            HIPCHK(hipMemcpyAsync(*d, v.data(), v.size() * sizeof v[0], hipMemcpyHostToDevice, s));
            return RV_OK;
        };
        int rc;
        if ((rc = up(cc.assert_rec2, &c->d_assert_rec2)) || (rc = up(cc.assert_op2, &c->d_assert_op2)) || (rc = up(cc.assert_rec64, &c->d_assert_rec64)) ||
            (rc = up(cc.assert_op64, &c->d_assert_op64)))
            return rc;
        HIPCHK(hipStreamSynchronize(s));
        c->assert_tables_up = true;
    }
    *f = EvalFold{};
    f->rec2 = c->d_assert_rec2, f->op2 = c->d_assert_op2, f->n2 = (uint32_t)cc.assert_rec2.size();
    f->rec64 = c->d_assert_rec64, f->op64 = c->d_assert_op64, f->n64 = (uint32_t)cc.assert_rec64.size();
    return RV_OK;
}

// one part of a batch that fits in device memory (witnesses in device memory are read where they lie; results for the device are
// written where they go, without a host wait: the caller synchronises once, behind the last part)
static int eval_part(rv_ctx* ctx, const rv_circuit* c, size_t B, const WitSrc& w, const EvalDst& o) {
    const Compiled& cc = c->cc;
    const uint8_t* const wit_gf2 = w.gf2;
    const uint64_t* const wit_z64 = w.z64;
    uint8_t* const gf2_values = o.gf2_values;
    uint64_t* const z64_values = o.z64_values;
    rv_eval_status* const st = o.st;
    const size_t W = (B + 31) / 32, n_in = cc.n_in, n_in64 = cc.n_in64;
    // (values that pass through the block below: the host form's)
    const size_t nw2 = gf2_values && !o.dev ? o.n2 : 0, nw64 = z64_values && !o.dev ? o.n64 : 0;
    // device: one block, 256-byte aligned parts
    size_t off = 0;
    auto part = [&](size_t bytes) {
        const size_t at = off;
        off += (bytes + 255) & ~(size_t)255;
        return at;
    };
    const size_t o_val = part(cc.n_rows * W * 4), o_win = part(n_in * W * 4), o_v64 = part(cc.n_ssa64 * B * 8);
    auto r8 = [](size_t x) { return (x + 7) & ~(size_t)7; };
    const size_t in_wz = w.dev ? 0 : r8(B * n_in), in_bytes = w.dev ? 0 : in_wz + B * n_in64 * 8;  // [B][n_in] bytes, then [B][n_in64] words
    const size_t o_in = part(in_bytes);
    // n_failed, first2, first64 ([B] u32 each), then [B][nw2] bytes and [B][nw64] words
    const size_t out2_at = r8(3 * B * 4), out64_at = r8(out2_at + B * nw2), out_bytes = out64_at + B * nw64 * 8;
    const size_t o_out = part(out_bytes);
    uint8_t* d = nullptr;
    if (int rc = dalloc(ctx, off, &d)) return rc;
    struct Release {
        rv_ctx* ctx;
        void* p;
        ~Release() { ctx->release(p); }
    } release{ctx, d};
    // RV_EVAL_POISON=1 (tests): the block starts non-zero, so that a row read before anything writes it shows (read at every call)
    if (getenv("RV_EVAL_POISON") && atoi(getenv("RV_EVAL_POISON"))) HIPCHK(hipMemsetAsync(d, 0xA5, off, ctx->stream));
    hipStream_t s = ctx->stream;
    if (!w.dev) {
        // witnesses in through a page-locked slot (only the elements the Input gates consume)
        int slot = -1;
        uint8_t* h_in = ctx->open_slot(std::max<size_t>(in_bytes, 1), &slot);
        if (!h_in) return RV_E_NOMEM;
        for (size_t b = 0; b < B; b++) {
            if (n_in) memcpy(h_in + b * n_in, wit_gf2 + b * w.stride_gf2, n_in);
            if (n_in64) memcpy(h_in + in_wz + b * n_in64 * 8, wit_z64 + b * w.stride_z64, n_in64 * 8);
        }
        if (in_bytes) HIPCHK(hipMemcpyAsync(d + o_in, h_in, in_bytes, hipMemcpyHostToDevice, s));
        HIPCHK(hipEventRecord(ctx->ev_open[slot], s));
    }
    wit_count(w, B * (n_in + n_in64 * 8));
    EvalParams p{};
    p.B = (uint32_t)B;
    p.W = (uint32_t)W;
    p.val = (uint32_t*)(d + o_val);
    p.win = (const uint32_t*)(d + o_win);
    p.v64 = (uint64_t*)(d + o_v64);
    p.wz = w.dev ? wit_z64 : (const uint64_t*)(d + o_in + in_wz);
    p.wz_stride = w.dev ? w.stride_z64 : n_in64;
    p.n_failed = (uint32_t*)(d + o_out);
    p.first2 = p.n_failed + B;
    p.first64 = p.first2 + B;
    HIPCHK(hipMemsetAsync(p.val + cc.zero_row * W, 0, W * 4, s));  // the zero row (never-written wires, unused operand slots)
    HIPCHK(hipMemsetAsync(p.v64, 0, B * 8, s));                   // Z64 SSA id 0
    HIPCHK(hipMemsetAsync(p.n_failed, 0, B * 4, s));
    HIPCHK(hipMemsetAsync(p.first2, 0xFF, 2 * B * 4, s));
    launch_eval_wit(s, w.dev ? wit_gf2 : d + o_in, w.dev ? w.stride_gf2 : n_in, (uint32_t)n_in, (uint32_t)B, (uint32_t)W, (uint32_t*)p.win);
    const uint32_t* d_ls64 = nullptr;
    if (eval_walks(cc) && !cc.gates64.empty()) {
        std::lock_guard<std::mutex> lk(c->eval_mu);
        if (!c->d_level_start64) {
            uint32_t* t = nullptr;
            if (int rc = dalloc(ctx, cc.level_start64.size(), &t)) return rc;
            HIPCHK(hipMemcpyAsync(t, cc.level_start64.data(), cc.level_start64.size() * 4, hipMemcpyHostToDevice, s));
            HIPCHK(hipStreamSynchronize(s));
            c->d_level_start64 = t;
        }
        d_ls64 = c->d_level_start64;
    }
    eval_run_levels(s, p, cc, c->d_gates, c->d_level_range, c->d_gates64, d_ls64);
    if (o.dev) {
        EvalFold f;
        if (int rc = eval_assert_tables(ctx, c, &f)) return rc;
        launch_eval_out_sel(s, p, c->d_wire_forms, o.d_sel2, (uint32_t)o.n2, c->d_wire_ssa64, o.d_sel64, (uint32_t)o.n64, o.n2 ? gf2_values : nullptr,
                            o.n64 ? z64_values : nullptr);
        launch_eval_status(s, p, f, st);
        HIPCHK(hipGetLastError());
        return RV_OK;
    }
    uint8_t* d_out2 = nw2 ? d + o_out + out2_at : nullptr;
    uint64_t* d_out64 = nw64 ? (uint64_t*)(d + o_out + out64_at) : nullptr;
    launch_eval_out(s, p, c->d_wire_forms, (uint32_t)nw2, c->d_wire_ssa64, (uint32_t)nw64, d_out2, d_out64);
    HIPCHK(hipGetLastError());
    int oslot = -1;
    uint8_t* h_out = ctx->open_slot(out_bytes, &oslot);
    if (!h_out) return RV_E_NOMEM;
    HIPCHK(hipMemcpyAsync(h_out, d + o_out, out_bytes, hipMemcpyDeviceToHost, s));
    HIPCHK(hipEventRecord(ctx->ev_open[oslot], s));
    HIPCHK(hipStreamSynchronize(s));
    g_wit_traffic[2].fetch_add(out_bytes, std::memory_order_relaxed);
    const uint32_t* nf = (const uint32_t*)h_out;
    for (size_t b = 0; b < B; b++) {
        st[b].n_failed = nf[b];
        st[b].first_failed_op = std::min(eval_assert_op(cc.assert_rec2, cc.assert_op2, nf[B + b]), eval_assert_op(cc.assert_rec64, cc.assert_op64, nf[2 * B + b]));
    }
    if (nw2) memcpy(gf2_values, h_out + out2_at, B * nw2);
    if (nw64) memcpy(z64_values, h_out + out64_at, B * nw64 * 8);
    return RV_OK;
}

// The refusals of both evaluator entry points that depend on the circuit and the witness lengths alone (nothing is launched)
static int eval_args_ok(const rv_circuit* c, const WitSrc& w, bool values) {
    const Compiled& cc = c->cc;
    if (values && !c->keep_wires) return RV_E_ARG;
    if (cc.n_user_random) return RV_E_UNSUPPORTED;  // (a Random wire has no single cleartext value)
    if (w.n_gf2 < cc.n_in || w.n_z64 < cc.n_in64) return RV_E_WITNESS_SHORT;
    if ((cc.n_in && !w.gf2) || (cc.n_in64 && !w.z64)) return RV_E_ARG;
    return RV_OK;
}

// o.n2 / o.n64: the values per witness of each domain (the caller's: every wire, or the selection's length)
static int rv_evaluate_batch_impl(rv_ctx* ctx, const rv_circuit* c, size_t batch, const WitSrc& w, const EvalDst& o) {
    LibBusy busy_guard;
    if (!ctx || !c || !o.st || !batch) return RV_E_ARG;
    const Compiled& cc = c->cc;
    if (int rc = eval_args_ok(c, w, o.gf2_values || o.z64_values)) return rc;
    HIPCHK(hipSetDevice(ctx->device));
    // parts of what fits in half of the free device memory (as rv_prove_batch), whole witness words each
    size_t free_b = 0, total_b = 0;
    if (hipMemGetInfo(&free_b, &total_b) != hipSuccess) return RV_E_DEVICE;
    const size_t nw2 = o.gf2_values ? o.n2 : 0, nw64 = o.z64_values ? o.n64 : 0;
    const size_t per32 = cc.n_rows * 4 + cc.n_in * 4 + 32 * (cc.n_ssa64 * 8 + cc.n_in + cc.n_in64 * 8 + 12 + nw2 + nw64 * 8);
    size_t part = std::max<size_t>((free_b + ctx->cached_bytes) / 2 / std::max<size_t>(per32, 1), 1) * 32;
    // RV_EVAL_PART=n (tests): parts of at most n witnesses, rounded up to whole words (read at every call)
    if (const char* e = getenv("RV_EVAL_PART")) part = std::min(part, ((size_t)std::max(atoll(e), 1LL) + 31) / 32 * 32);
    for (size_t b0 = 0; b0 < batch; b0 += part) {
        const size_t n = std::min(part, batch - b0);
        const int rc = eval_part(ctx, c, n, w.from(b0), o.from(b0));
        if (rc) return rc;
    }
    if (o.dev) HIPCHK(hipStreamSynchronize(ctx->stream));  // (the device form's one wait: the witnesses are no longer read, the results are there)
    return RV_OK;
}

extern "C" int rv_evaluate_batch(rv_ctx* ctx, const rv_circuit* c, size_t batch, const uint8_t* wit_gf2, size_t n_gf2, const uint64_t* wit_z64,
                                 size_t n_z64, uint8_t* gf2_values, uint64_t* z64_values, rv_eval_status* st) {
    try {
        if (!c) return RV_E_ARG;
        return rv_evaluate_batch_impl(ctx, c, batch, wit_host(wit_gf2, n_gf2, wit_z64, n_z64),
                                      EvalDst{gf2_values, z64_values, st, c->cc.wire_forms.size(), c->cc.wire_ssa64.size(), false, nullptr, nullptr});
    } catch (...) {
        g_last_error = "out of host memory";
        return RV_E_NOMEM;
    }
}

extern "C" int rv_evaluate(rv_ctx* ctx, const rv_circuit* c, const uint8_t* wit_gf2, size_t n_gf2, const uint64_t* wit_z64, size_t n_z64,
                           uint8_t* gf2_values, uint64_t* z64_values, rv_eval_status* st) {
    return rv_evaluate_batch(ctx, c, 1, wit_gf2, n_gf2, wit_z64, n_z64, gf2_values, z64_values, st);
}

extern "C" int rv_hook_eval_schedules(uint64_t out[2]) {
    if (!out) return RV_E_ARG;
    out[0] = g_eval_sched[0].load();
    out[1] = g_eval_sched[1].load();
    return RV_OK;
}
