// rv_eval_stream_*: cleartext evaluation of a gate stream fed in pieces, with bounded device memory (kernels: eval.hip).
// Included by api.hip after eval.inc.
//
// Each piece is compiled as a streaming chunk (compile.h, ChunkStart): it starts from the carried GF(2) rows [0, gf2_wires) and Z64
// SSA slots 1 + w, and ends with a write-back level of G_XORK / G64_ADDC copies into them.  The evaluator keeps those carried
// rows and slots as the wire store of VALUES:
//   val[row][W] u32 (W = ceil(B / 32)): carried rows 0 .. gf2_wires - 1 first, then the chunk's mask and computed rows (scratch);
//   v64[ssa][B] u64: SSA 0 (the zero wire), carried slots 1 .. z64_wires, then the chunk's SSA ids (scratch).
// Mask phases and transcript offsets do not matter for values: every piece is compiled at zero.  A chunk runs as a compiled circuit
// does in eval_part (launch_eval_wit, eval_run_levels), then k_eval_fold folds its failing assertions into the stream's per-witness
// status (first failing op index, total count: O(B) words whatever the number of chunks).  Nothing waits for the GPU per chunk:
// the host compiles the next pieces on worker threads while a chunk runs; a page-locked slot is waited for only when it is reused.

struct rv_eval_stream {
    rv_ctx* ctx = nullptr;
    size_t z64_wires = 0, gf2_wires = 0, B = 0, W = 0;
    size_t max_chunk_ops = (size_t)1 << 18;
    int sticky = RV_OK;  // first error: only abort from here on
    bool finished = false;
    uint32_t compile_flags = 0;  // rv_eval_stream_set_compile_flags (the context's at the begin): RV_COMPILE_DEVICE, as rv_stream's
    bool fed = false;
    uint32_t* d_val = nullptr;  // [rows_cap][W]
    size_t rows_cap = 0;
    uint64_t* d_v64 = nullptr;  // [ssa64_cap][B]
    size_t ssa64_cap = 0;
    uint8_t* d_st = nullptr;  // first_op [B] u64, total [B] u64, then the chunk's n_failed, first2, first64 [B] u32 each
    uint64_t n_ops = 0, chunks = 0, levels = 0, peak_chunk = 0;
    uint64_t* first_op() const { return (uint64_t*)d_st; }
    uint64_t* total() const { return (uint64_t*)d_st + B; }
    uint32_t* n_failed() const { return (uint32_t*)((uint64_t*)d_st + 2 * B); }
    static size_t status_bytes(size_t B) { return B * 28; }
    size_t store_bytes() const { return gf2_wires * W * 4 + (1 + z64_wires) * B * 8 + status_bytes(B); }
    void free_all() {
        ctx->release(d_val);
        ctx->release(d_v64);
        ctx->release(d_st);
        d_val = nullptr, d_v64 = nullptr, d_st = nullptr;
    }
};

extern "C" void rv_eval_stream_abort(rv_eval_stream* E) {
    if (!E) return;
    (void)hipSetDevice(E->ctx->device);
    (void)hipStreamSynchronize(E->ctx->stream);
    E->free_all();
    delete E;
}

static int eval_stream_begin_impl(rv_ctx* ctx, size_t z64_wires, size_t gf2_wires, size_t batch, size_t max_chunk_ops, rv_eval_stream** out) {
    if (!ctx || !out || !batch) return RV_E_ARG;
    *out = nullptr;
    // (row / slot ids are 32-bit, with the compiler's flag bits above 2^30; EvalParams::B is 32-bit)
    if (gf2_wires > 0x3FFFFFFFull || z64_wires > 0x3FFFFFFFull || batch > 0x7FFFFFFFull) return RV_E_UNSUPPORTED;
    HIPCHK(hipSetDevice(ctx->device));
    const size_t W = (batch + 31) / 32;
    // the wire store in half of the free device memory (plus what the context's arena holds idle), checked before anything is allocated
    const double want = (double)gf2_wires * W * 4 + (double)(1 + z64_wires) * batch * 8 + (double)rv_eval_stream::status_bytes(batch);
    size_t free_b = 0, total_b = 0;
    if (hipMemGetInfo(&free_b, &total_b) != hipSuccess) return RV_E_DEVICE;
    if (want > ((double)free_b + (double)ctx->cached_bytes) / 2) {
        g_last_error = "the wire store of the streaming evaluation does not fit in half of the free device memory";
        return RV_E_NOMEM;
    }
    rv_eval_stream* E = new rv_eval_stream();
    E->ctx = ctx;
    E->z64_wires = z64_wires;
    E->gf2_wires = gf2_wires;
    E->B = batch;
    E->W = W;
    E->compile_flags = ctx->compile_flags & RV_COMPILE_DEVICE_BITS;
    if (max_chunk_ops) E->max_chunk_ops = max_chunk_ops;
    int rc;
    E->rows_cap = std::max<size_t>(gf2_wires, 1);
    E->ssa64_cap = 1 + z64_wires;
    if ((rc = dalloc(ctx, E->rows_cap * W, &E->d_val)) || (rc = dalloc(ctx, E->ssa64_cap * batch, &E->d_v64)) ||
        (rc = dalloc(ctx, rv_eval_stream::status_bytes(batch), &E->d_st))) {
        rv_eval_stream_abort(E);
        return rc;
    }
    // every wire starts as zero (interpreter/single.rs:16); no failures yet
    hipStream_t s = ctx->stream;
    if (hipMemsetAsync(E->d_val, 0, E->rows_cap * W * 4, s) != hipSuccess || hipMemsetAsync(E->d_v64, 0, E->ssa64_cap * batch * 8, s) != hipSuccess ||
        hipMemsetAsync(E->d_st, 0xFF, batch * 8, s) != hipSuccess || hipMemsetAsync(E->d_st + batch * 8, 0, batch * 12, s) != hipSuccess ||
        hipMemsetAsync(E->d_st + batch * 20, 0xFF, batch * 8, s) != hipSuccess) {
        const int code = hip_fail(hipGetLastError(), "eval stream begin", __FILE__, __LINE__);
        rv_eval_stream_abort(E);
        return code;
    }
    *out = E;
    return RV_OK;
}

extern "C" int rv_eval_stream_begin(rv_ctx* ctx, size_t z64_wires, size_t gf2_wires, size_t batch, size_t max_chunk_ops, rv_eval_stream** out) {
    return guarded([&] { return eval_stream_begin_impl(ctx, z64_wires, gf2_wires, batch, max_chunk_ops, out); });
}

extern "C" int rv_eval_stream_set_compile_flags(rv_eval_stream* E, uint32_t flags) {
    if (int rc = check_device_flags("rv_eval_stream_set_compile_flags", flags)) return rc;
    if (!E || E->fed) return RV_E_ARG;
    E->compile_flags = flags;
    return RV_OK;
}

// value rows / SSA slots for a chunk: a larger block, the carried prefix copied over on the stream (the old block goes back to the arena;
// the stream's order keeps its reuse behind the kernels that still read it)
static int eval_stream_reserve(rv_eval_stream* E, const Compiled& cc) {
    rv_ctx* ctx = E->ctx;
    hipStream_t s = ctx->stream;
    int rc;
    if (cc.n_rows > E->rows_cap) {
        const size_t cap = std::max<size_t>(cc.n_rows, E->rows_cap + E->rows_cap / 2);
        uint32_t* v = nullptr;
        if ((rc = dalloc(ctx, cap * E->W, &v))) return rc;
        HIPCHK(hipMemcpyAsync(v, E->d_val, std::max<size_t>(E->gf2_wires, 1) * E->W * 4, hipMemcpyDeviceToDevice, s));
        ctx->release(E->d_val);
        E->d_val = v;
        E->rows_cap = cap;
    }
    if (cc.n_ssa64 > E->ssa64_cap) {
        const size_t cap = std::max<size_t>(cc.n_ssa64, E->ssa64_cap + E->ssa64_cap / 2);
        uint64_t* v = nullptr;
        if ((rc = dalloc(ctx, cap * E->B, &v))) return rc;
        HIPCHK(hipMemcpyAsync(v, E->d_v64, (1 + E->z64_wires) * E->B * 8, hipMemcpyDeviceToDevice, s));
        ctx->release(E->d_v64);
        E->d_v64 = v;
        E->ssa64_cap = cap;
    }
    return RV_OK;
}

// the witness rows of a feed: witness b's n_gf2 / n_z64 elements at gf2 + b * stride2, z64 + b * stride64 (elements); dev: in the
// memory of the stream's device (rv_eval_stream_feed_wdev)
struct EvalWitRows {
    const uint8_t* gf2;
    size_t n_gf2, stride2;
    const uint64_t* z64;
    size_t n_z64, stride64;
    bool dev;
};

// One compiled chunk on the device.  op_base: the index of its first op in the whole op list.  The chunk consumes witness elements
// [*u2, *u2 + n_in) and [*u64, *u64 + n_in64) of every witness row of the feed and advances *u2 / *u64.  Host rows are staged
// with the chunk's tables; device rows go into the same input area by one strided device-to-device copy per domain.
static int eval_stream_chunk(rv_eval_stream* E, const Compiled& cc, uint64_t op_base, const EvalWitRows& wit, size_t* u2, size_t* u64) {
    if (cc.n_user_random) return RV_E_UNSUPPORTED;  // (a Random wire has no single cleartext value)
    const size_t n_in = cc.n_in, n_in64 = cc.n_in64, B = E->B, W = E->W;
    if (wit.n_gf2 - *u2 < n_in || wit.n_z64 - *u64 < n_in64) return RV_E_WITNESS_SHORT;
    rv_ctx* ctx = E->ctx;
    hipStream_t s = ctx->stream;
    if (int rc = eval_stream_reserve(E, cc)) return rc;
    // the chunk's block: [gate records and tables, witness slices] (staged through a page-locked slot, one copy), then the
    // bit-sliced input words (device only)
    const bool has64 = !cc.gates64.empty();
    size_t off = 0;
    auto part = [&](size_t bytes) {
        const size_t at = off;
        off += (bytes + 255) & ~(size_t)255;
        return at;
    };
    const size_t n2 = cc.assert_rec2.size(), n64 = cc.assert_rec64.size();
    const size_t o_g = part(cc.gates.size() * sizeof(Gate)), o_lr = part(cc.level_range.size() * sizeof(LevelRange)),
                 o_g64 = part(cc.gates64.size() * sizeof(Gate64)), o_ls64 = part(has64 ? cc.level_start64.size() * 4 : 0),
                 o_r2 = part(n2 * 4), o_op2 = part(n2 * 8), o_r64 = part(n64 * 4), o_op64 = part(n64 * 8);
    const size_t tables = off;
    const size_t o_wz = part(B * n_in64 * 8), o_w2 = part(B * n_in);
    const size_t staged = wit.dev ? tables : off;
    const size_t o_win = part(n_in * W * 4);
    const size_t block = off;
    // the chunk's working set beside the wire store (rv_eval_stream_info::peak_chunk_bytes)
    const uint64_t work = (cc.n_rows - E->gf2_wires) * W * 4 + (cc.n_ssa64 - 1 - E->z64_wires) * B * 8 + block;
    E->peak_chunk = std::max(E->peak_chunk, work);
    uint8_t* d = nullptr;
    if (int rc = dalloc(ctx, block, &d)) return rc;
    struct Release {
        rv_ctx* ctx;
        void* p;
        ~Release() { ctx->release(p); }  // (stream order: the next chunk's copies into it come after this chunk's kernels)
    } release{ctx, d};
    int slot = -1;
    uint8_t* h = ctx->open_slot(std::max<size_t>(staged, 1), &slot);  // (waits only if the slot's previous copy is still in flight)
    if (!h) return RV_E_NOMEM;
    auto put = [&](size_t at, const void* src, size_t bytes) {
        if (bytes) memcpy(h + at, src, bytes);
    };
    put(o_g, cc.gates.data(), cc.gates.size() * sizeof(Gate));
    put(o_lr, cc.level_range.data(), cc.level_range.size() * sizeof(LevelRange));
    put(o_g64, cc.gates64.data(), cc.gates64.size() * sizeof(Gate64));
    if (has64) put(o_ls64, cc.level_start64.data(), cc.level_start64.size() * 4);
    put(o_r2, cc.assert_rec2.data(), n2 * 4);
    put(o_op2, cc.assert_op2.data(), n2 * 8);
    put(o_r64, cc.assert_rec64.data(), n64 * 4);
    put(o_op64, cc.assert_op64.data(), n64 * 8);
    for (size_t b = 0; b < B && !wit.dev; b++) {
        if (n_in64) memcpy(h + o_wz + b * n_in64 * 8, wit.z64 + b * wit.stride64 + *u64, n_in64 * 8);
        if (n_in) memcpy(h + o_w2 + b * n_in, wit.gf2 + b * wit.stride2 + *u2, n_in);
    }
    if (staged) HIPCHK(hipMemcpyAsync(d, h, staged, hipMemcpyHostToDevice, s));
    HIPCHK(hipEventRecord(ctx->ev_open[slot], s));
    if (wit.dev) {
        if (n_in64)
            HIPCHK(hipMemcpy2DAsync(d + o_wz, n_in64 * 8, wit.z64 + *u64, (B > 1 ? wit.stride64 : n_in64) * 8, n_in64 * 8, B, hipMemcpyDeviceToDevice, s));
        if (n_in) HIPCHK(hipMemcpy2DAsync(d + o_w2, n_in, wit.gf2 + *u2, B > 1 ? wit.stride2 : n_in, n_in, B, hipMemcpyDeviceToDevice, s));
    }
    stream_traffic(wit.dev ? 1 : 0, B * (n_in + n_in64 * 8));
    // RV_EVAL_POISON=1 (tests): the chunk's scratch rows and slots start non-zero, never the carried store (read at every call)
    if (getenv("RV_EVAL_POISON") && atoi(getenv("RV_EVAL_POISON"))) {
        HIPCHK(hipMemsetAsync(E->d_val + E->gf2_wires * W, 0xA5, (cc.n_rows - E->gf2_wires) * W * 4, s));
        HIPCHK(hipMemsetAsync(E->d_v64 + (1 + E->z64_wires) * B, 0xA5, (cc.n_ssa64 - 1 - E->z64_wires) * B * 8, s));
        HIPCHK(hipMemsetAsync(d + o_win, 0xA5, block - o_win, s));
    }
    EvalParams p{};
    p.B = (uint32_t)B;
    p.W = (uint32_t)W;
    p.val = E->d_val;
    p.win = (const uint32_t*)(d + o_win);
    p.v64 = E->d_v64;
    p.wz = (const uint64_t*)(d + o_wz);
    p.wz_stride = n_in64;
    p.n_failed = E->n_failed();
    p.first2 = p.n_failed + B;
    p.first64 = p.first2 + B;
    HIPCHK(hipMemsetAsync(p.val + cc.zero_row * W, 0, W * 4, s));  // the chunk's zero row (unused operand slots)
    launch_eval_wit(s, d + o_w2, n_in, (uint32_t)n_in, (uint32_t)B, (uint32_t)W, (uint32_t*)p.win);
    eval_run_levels(s, p, cc, (const Gate*)(d + o_g), (const LevelRange*)(d + o_lr), (const Gate64*)(d + o_g64), (const uint32_t*)(d + o_ls64));
    EvalFold f{};
    f.rec2 = (const uint32_t*)(d + o_r2);
    f.op2 = (const uint64_t*)(d + o_op2);
    f.rec64 = (const uint32_t*)(d + o_r64);
    f.op64 = (const uint64_t*)(d + o_op64);
    f.n2 = (uint32_t)n2;
    f.n64 = (uint32_t)n64;
    f.op_base = op_base;
    f.first_op = E->first_op();
    f.total = E->total();
    launch_eval_fold(s, p, f);
    HIPCHK(hipGetLastError());
    *u2 += n_in;
    *u64 += n_in64;
    E->chunks++;
    E->levels += cc.level_range.size();
    return RV_OK;
}

// worker threads of a feed: the CPUs this process may use, at most 16 (oversubscribed compile threads throttle the GPU's feeder)
static unsigned eval_stream_threads() { return std::min(cpu_budget(), 16u); }

// ops_on_device: `ops` is in the memory of the stream's device (rv_eval_stream_feed_device; feed_ops.inc)
static int eval_stream_feed_impl(rv_eval_stream* E, const rv_op* ops, bool ops_on_device, size_t n_ops, const EvalWitRows& wit) {
    LibBusy busy_guard;
    if (!E) return RV_E_ARG;
    if (E->sticky) return E->sticky;
    if (E->finished || (n_ops && !ops) || (wit.n_gf2 && !wit.gf2) || (wit.n_z64 && !wit.z64) || (ops_on_device && ((uintptr_t)ops & 7))) return E->sticky = RV_E_ARG;
    E->fed = true;
    HIPCHK(hipSetDevice(E->ctx->device));
    const std::vector<size_t> cut = stream_cuts(n_ops, E->max_chunk_ops);  // (the streaming prover's rule)
    const size_t n_pieces = cut.size() - 1;
    const uint64_t first_op = E->n_ops;
    size_t u2 = 0, u64 = 0;
    // the pieces are compiled ahead on worker threads and run in order (piece_pipe.h)
    const unsigned n_threads = (unsigned)std::min<size_t>(eval_stream_threads(), n_pieces);
    std::vector<std::unique_ptr<Compiled>> pieces(n_pieces);
    const ChunkStart cs;  // (values do not depend on mask phases or transcript offsets)
    FeedOps fo(E->ctx, ops, ops_on_device && n_ops, cut);
    if (int rs = fo.load_sums(first_op, n_threads)) return E->sticky = rs;
    auto compile_on_host = [&](size_t i) {
        const PieceOnHost h(fo, i);
        return h.rc() ? h.rc() : compile_ops(h.ops(), fo.len(i), E->z64_wires, E->gf2_wires, *pieces[i], &cs);
    };
    PiecePipe pipe(n_pieces, n_threads, RV_E_NOMEM, [&](size_t i) {
        // (RV_COMPILE_DEVICE: an all-GF(2) piece -- under RV_COMPILE_DEVICE_Z64 any piece without B2A, with RV_COMPILE_DEVICE_B2A any piece -- stays empty here: the main
        // thread compiles it on the GPU right before it runs)
        if (fo.for_device(i, E->compile_flags)) return (int)RV_OK;
        pieces[i].reset(new Compiled());
        return compile_on_host(i);
    });
    int rc = RV_OK;
    for (size_t i = 0; i < n_pieces && !rc; i++) {
        rc = pipe.wait(i);
        if (!rc && !pieces[i]) {
            // (the piece comes back to the host whole: the chunk's arrays go up in one block with its witness, eval_stream_chunk)
            pieces[i].reset(new Compiled());
            const int rd = fo.compile_on_device(i, E->z64_wires, E->gf2_wires, cs, *pieces[i], nullptr, nullptr, E->compile_flags);
            if (rd == RV_OK) g_stream_device_chunks.fetch_add(1, std::memory_order_relaxed);
            rc = rd == RV_COMPILE_FALLBACK ? compile_on_host(i) : rd;
        }
        if (!rc) rc = eval_stream_chunk(E, *pieces[i], first_op + cut[i], wit, &u2, &u64);
        pieces[i].reset();  // (host memory of the compiled piece: freed here, on the main thread, while the GPU runs it)
        pipe.consumed(i, rc);
    }
    if (rc) return E->sticky = rc;
    E->n_ops += n_ops;
    return RV_OK;
}

extern "C" int rv_eval_stream_feed(rv_eval_stream* E, const rv_op* ops, size_t n_ops, const uint8_t* wit_gf2, size_t n_gf2, const uint64_t* wit_z64,
                                   size_t n_z64) {
    const int rc = guarded([&] { return eval_stream_feed_impl(E, ops, false, n_ops, EvalWitRows{wit_gf2, n_gf2, n_gf2, wit_z64, n_z64, n_z64, false}); });
    if (rc == RV_E_NOMEM && E) E->sticky = rc;  // (a thrown one too: the stream is dead after any failed allocation)
    return rc;
}

extern "C" int rv_eval_stream_feed_device(rv_eval_stream* E, const rv_op* d_ops, size_t n_ops, const uint8_t* wit_gf2, size_t n_gf2,
                                          const uint64_t* wit_z64, size_t n_z64) {
    // (every read of d_ops has finished when this returns: the device compiles and the copies down are waited for)
    const int rc = guarded([&] { return eval_stream_feed_impl(E, d_ops, true, n_ops, EvalWitRows{wit_gf2, n_gf2, n_gf2, wit_z64, n_z64, n_z64, false}); });
    if (rc == RV_E_NOMEM && E) E->sticky = rc;
    return rc;
}

static int eval_stream_finish_impl(rv_eval_stream* E, uint8_t* gf2_values, uint64_t* z64_values, rv_eval_status* st) {
    LibBusy busy_guard;
    if (!E) return RV_E_ARG;
    if (E->sticky) return E->sticky;
    if (E->finished || !st) return E->sticky = RV_E_ARG;
    E->finished = true;
    rv_ctx* ctx = E->ctx;
    hipStream_t s = ctx->stream;
    HIPCHK(hipSetDevice(ctx->device));
    const size_t B = E->B, n2 = gf2_values ? E->gf2_wires : 0, n64 = z64_values ? E->z64_wires : 0;
    // the final values, a group of witnesses at a time through a device buffer of at most 64 MiB
    if (n2 + n64) {
        const size_t per = n2 + n64 * 8, group = std::max<size_t>(std::min<size_t>(B, ((size_t)64 << 20) / per), 1);
        const size_t o64 = (group * n2 + 255) & ~(size_t)255;
        uint8_t* d = nullptr;
        if (int rc = dalloc(ctx, o64 + group * n64 * 8, &d)) return E->sticky = rc;
        struct Release {
            rv_ctx* ctx;
            void* p;
            ~Release() { ctx->release(p); }
        } release{ctx, d};
        EvalParams p{};
        p.B = (uint32_t)B;
        p.W = (uint32_t)E->W;
        p.val = E->d_val;
        p.v64 = E->d_v64;
        for (size_t b0 = 0; b0 < B; b0 += group) {
            const size_t nb = std::min(group, B - b0);
            launch_eval_stream_out(s, p, (uint32_t)n2, (uint32_t)n64, (uint32_t)b0, (uint32_t)nb, n2 ? d : nullptr, n64 ? (uint64_t*)(d + o64) : nullptr);
            HIPCHK(hipGetLastError());
            if (n2) HIPCHK(hipMemcpyAsync(gf2_values + b0 * n2, d, nb * n2, hipMemcpyDeviceToHost, s));
            if (n64) HIPCHK(hipMemcpyAsync(z64_values + b0 * n64, d + o64, nb * n64 * 8, hipMemcpyDeviceToHost, s));
            HIPCHK(hipStreamSynchronize(s));
        }
    }
    std::vector<uint64_t> h(2 * B);
    HIPCHK(hipMemcpyAsync(h.data(), E->d_st, 2 * B * 8, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    for (size_t b = 0; b < B; b++) {
        st[b].first_failed_op = h[b];
        st[b].n_failed = h[B + b];
    }
    return RV_OK;
}

extern "C" int rv_eval_stream_finish(rv_eval_stream* E, uint8_t* gf2_values, uint64_t* z64_values, rv_eval_status* st) {
    const int rc = guarded([&] { return eval_stream_finish_impl(E, gf2_values, z64_values, st); });
    if (rc == RV_E_NOMEM && E) E->sticky = rc;  // (a thrown one too: the stream is dead after any failed allocation)
    return rc;
}

extern "C" int rv_eval_stream_get_info(const rv_eval_stream* E, rv_eval_stream_info* info) {
    if (!E || !info) return RV_E_ARG;
    *info = rv_eval_stream_info{};
    info->n_ops = E->n_ops;
    info->chunks = E->chunks;
    info->levels = E->levels;
    info->wire_store_bytes = E->store_bytes();
    info->peak_chunk_bytes = E->peak_chunk;
    return RV_OK;
}

extern "C" int rv_evaluate_streaming(rv_ctx* ctx, const rv_op* ops, size_t n_ops, size_t z64_wires, size_t gf2_wires, size_t batch,
                                     const uint8_t* wit_gf2, size_t n_gf2, const uint64_t* wit_z64, size_t n_z64, size_t max_chunk_ops,
                                     uint8_t* gf2_values, uint64_t* z64_values, rv_eval_status* st, rv_eval_stream_info* info) {
    if (!st) return RV_E_ARG;
    rv_eval_stream* E = nullptr;
    int rc = rv_eval_stream_begin(ctx, z64_wires, gf2_wires, batch, max_chunk_ops, &E);
    if (rc) return rc;
    rc = rv_eval_stream_feed(E, ops, n_ops, wit_gf2, n_gf2, wit_z64, n_z64);
    if (!rc) rc = rv_eval_stream_finish(E, gf2_values, z64_values, st);
    if (info) rv_eval_stream_get_info(E, info);
    rv_eval_stream_abort(E);
    return rc;
}
