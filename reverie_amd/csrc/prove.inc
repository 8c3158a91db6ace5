// Part of api.hip (#included there, one translation unit): the single-proof prover (DESIGN.md section 9.2) -- what a call decides
// (ProveSchedule), the commitment (rv_shard_commit), Proof::new (proof/mod.rs:119-222) as a pipeline in steps (ProveRun: rv_prove,
// with the early-corrections path) and the forms that leave the proof in device memory (rv_prove_device).

// What one call of the single-proof prover decides about its own work, from the circuit and the environment -- every knob is read
// when it always was: RV_VCLR and RV_AES_COL4 once per process, RV_EARLY_MIN / _CHUNKS / _REPS once per circuit (early_plan), the
// others at every call (tests and tools switch them).  The first group belongs to the commitment and is decided for every caller of
// rv_shard_commit_impl; the second only for rv_prove_impl (host_proof), and two of its fields are settled by later steps of ProveRun:
// `early` falls back when the proof's buffer cannot be had or mapped, `stage_out` when the mapped staging buffer cannot.
struct ProveSchedule {
    bool stage_in;     // seeds and GF(2) witness in ONE copy through the page-locked input staging buffer
    bool vclr;         // MODE_PROVE_V: cleartext values instead of corr rows (internal.h)
    bool z64f;         // the fused Z64 prover (internal.h: Z64FParams)
    bool overlap;      // the GF(2) mask generator beside the level launches (RV_OVERLAP, shard.inc)
    bool col4;         // the lane-distributed mask generator (aes_col4.hip)
    bool early;        // early corrections: the corrections vectors cross PCIe before the challenge exists
    bool early_z64;    // ... in their Z64 form (2-D copies of the preprocessing rows, nothing packed)
    OpenDirect od;     // ... n_direct != 0: that leading share of the broadcast vectors' tiles goes straight into the proof buffer
    bool stage_out;    // the framed proof through the context's mapped staging buffer, no copy engine
    const EarlyPlan* plan;
};
extern "C" int rv_hook_prove_schedule(uint64_t out[16]) {
    if (!out) return RV_E_ARG;
    for (int i = 0; i < 16; i++) out[i] = g_prove_schedule[i].load(std::memory_order_relaxed);
    return RV_OK;
}
// R repetitions in rows of R / 4 quad words; defer_sync: the caller waits for the stream itself before it returns, so the
// page-locked input staging buffer is free again by the next call.  host_proof: rv_prove_impl's call; may_early: ... which may
// take the early-corrections path (a one-shot rv_prove_ops does without: its staging buffer is 3x the proof of page-locked
// memory, tens of milliseconds to map for a gain of half a millisecond; a proof into the caller's buffer has no mapped address)
static ProveSchedule prove_schedule(rv_ctx* ctx, const rv_circuit* c, uint32_t R, bool defer_sync, bool host_proof, bool may_early) {
    const Compiled& cc = c->cc;
    const uint32_t NQ = R / 4;
    ProveSchedule v{};
    v.stage_in = defer_sync && (size_t)R * 16 + cc.n_in <= rv_ctx::IN_STAGE_BYTES &&
                 (ctx->h_in || hipHostMalloc((void**)&ctx->h_in, rv_ctx::IN_STAGE_BYTES, hipHostMallocDefault) == hipSuccess);
    if (!v.stage_in) (void)hipGetLastError();
    // eligible circuits (whole proofs and the repetition shards with a specialised interpreter)
    static const bool vclr_on = [] {
        const char* e = getenv("RV_VCLR");
        return !e || atoi(e) != 0;
    }();
    v.vclr = vclr_on && c->vclr_ok && (NQ == 64 || NQ == 32 || NQ == 16 || NQ == 8);
    v.z64f = c->z64f_ok && z64_fused_on() && z64_fused_supports(NQ) && !g_recorder;
    // the mask generator beside the level launches (RV_OVERLAP=0 turns it off; RV_OVERLAP_MIN = fewest CTR blocks): wide circuits
    // only -- a level must be long enough to hide a share of the cipher behind
    const int ov_mode = getenv("RV_OVERLAP") ? atoi(getenv("RV_OVERLAP")) : 1;  // (read at every call: bench.py and the tools switch it)
    const uint64_t ov_min = getenv("RV_OVERLAP_MIN") ? strtoull(getenv("RV_OVERLAP_MIN"), nullptr, 0) : 8192;  // (per call: the tests lower it)
    const uint64_t n_blocks = cc.n_masks_pad / 128;
    v.overlap = ov_mode != 0 && !g_recorder && aes_col4_supports(NQ) && n_blocks >= ov_min;
    v.col4 = gf2_masks_col4(NQ, n_blocks, v.overlap);
    v.overlap = v.overlap && v.col4;
    if (!host_proof || g_recorder) return v;
    // small proofs: the layout of a whole proof does not depend on the challenge, so its size is known before the openings exist
    const OpenLayout L = whole_proof_layout(cc);
    v.stage_out = L.total + 64 <= rv_ctx::STAGE_BYTES;
    const bool early_on = !(getenv("RV_EARLY") && atoi(getenv("RV_EARLY")) == 0);
    if (!early_on || !may_early || !early_plan(c)->ok) return v;
    v.plan = early_plan(c);
    v.early = true;
    v.early_z64 = v.plan->z64;
    v.stage_out = false;
    if (v.early_z64) return v;
    // The broadcast vectors go to the proof buffer from the extraction kernel itself (internal.h: OpenDirect; DESIGN.md section 9.1),
    // k_copy_gaps behind it brings the rest of the image.  By default where the vectors are long enough for tiles of 64 bytes and
    // more; RV_OPEN_DIRECT=num/den (read at every call: the tests switch it): only that leading share of the tiles (0/1: none),
    // and whatever the tile (16 bytes at least)
    unsigned num = 1, den = 1;
    const char* e = getenv("RV_OPEN_DIRECT");
    if (e && (sscanf(e, "%u/%u", &num, &den) != 2 || !den || num > den)) num = 0, den = 1;
    v.od.tile = extract_tile_bytes(cc.n_rec);
    v.od.rvec_at = 137;  // (k_fs_challenge: a record's broadcast vector follows its 129-byte head and an 8-byte length)
    v.od.rvec_len = L.l2r;
    v.od.n_direct = (uint32_t)(((L.l2r + v.od.tile - 1) / v.od.tile) * num / den);
    if (!v.od.n_direct || v.od.tile < (e ? 16u : 64u) || (v.od.tile & (v.od.tile - 1))) v.od = OpenDirect();
    return v;
}

// sch (nullable): what the caller's prove_schedule decided; otherwise the commitment decides for itself
// defer_sync: do not wait for the device (nor look at the invalid-witness flag): the caller queues more work behind
// the commitment and checks s->d_err itself after its own synchronisation
static int rv_shard_commit_impl(rv_ctx* ctx, const rv_circuit* c, const WitSrc& w, const uint8_t* seeds, uint32_t rep_begin, uint32_t rep_count,
                               rv_shard** out, bool defer_sync = false, EarlyRun* ec = nullptr, const ProveSchedule* sch = nullptr) {
    LibBusy busy_guard;  // (compile.h: the background unmapper keeps still while the GPU is driven)
    if (!ctx || !c || !out || !seeds) return RV_E_ARG;
    const uint8_t* const wit_gf2 = w.gf2;
    const uint64_t* const wit_z64 = w.z64;
    const size_t n_gf2 = w.n_gf2, n_z64 = w.n_z64;
    if (rep_count == 0 || rep_count % 8 || rep_begin % 8 || rep_begin + rep_count > RV_TOTAL_REPS) return RV_E_ARG;
    *out = nullptr;
    const Compiled& cc = c->cc;
    if (n_gf2 < cc.n_in || n_z64 < cc.n_in64) return RV_E_WITNESS_SHORT;
    if ((cc.n_in && !wit_gf2) || (cc.n_in64 && !wit_z64)) return RV_E_ARG;
    HIPCHK(hipSetDevice(ctx->device));
    const ProveSchedule v = sch ? *sch : prove_schedule(ctx, c, rep_count, defer_sync, false, false);
    rv_shard* s = new rv_shard();
    s->ctx = ctx;
    s->c = c;
    s->rep_begin = rep_begin;
    s->R = rep_count;
    s->NQ = rep_count / 4;
    int rc = RV_OK;
    auto fail = [&](int code) {
        rv_shard_destroy(s);
        return code;
    };
    const size_t seed_bytes = (size_t)s->R * 16;
    if (v.stage_in) {
        if ((rc = dalloc(ctx, seed_bytes + std::max<size_t>(cc.n_in, 1), &s->d_seeds)) || (rc = dalloc(ctx, (size_t)s->R * 128, &s->d_keys))) return fail(rc);
        s->d_wit = s->d_seeds + seed_bytes;  // (inside d_seeds' block: the arena ignores it on release)
        memcpy(ctx->h_in, seeds, seed_bytes);
        // (a witness in device memory: only the seeds are staged, the witness is copied behind them from where it lies)
        const size_t staged_wit = w.dev ? 0 : cc.n_in;
        if (staged_wit) memcpy(ctx->h_in + seed_bytes, wit_gf2, staged_wit);
        if (hipMemcpyAsync(s->d_seeds, ctx->h_in, seed_bytes + staged_wit, hipMemcpyHostToDevice, ctx->stream) != hipSuccess) return fail(RV_E_DEVICE);
        if (w.dev && cc.n_in && hipMemcpyAsync(s->d_wit, wit_gf2, cc.n_in, hipMemcpyDeviceToDevice, ctx->stream) != hipSuccess) return fail(RV_E_DEVICE);
    } else {
        if ((rc = dalloc(ctx, seed_bytes, &s->d_seeds)) || (rc = dalloc(ctx, (size_t)s->R * 128, &s->d_keys)) ||
            (rc = dalloc(ctx, std::max<size_t>(cc.n_in, 1), &s->d_wit)))
            return fail(rc);
        if (hipMemcpyAsync(s->d_seeds, seeds, seed_bytes, hipMemcpyHostToDevice, ctx->stream) != hipSuccess) return fail(RV_E_DEVICE);
        if (cc.n_in && hipMemcpyAsync(s->d_wit, wit_gf2, cc.n_in, w.kind(), ctx->stream) != hipSuccess) return fail(RV_E_DEVICE);
    }
    if (cc.n_in64) {
        if ((rc = dalloc(ctx, cc.n_in64, &s->d_wit64))) return fail(rc);
        if (hipMemcpyAsync(s->d_wit64, wit_z64, cc.n_in64 * 8, w.kind(), ctx->stream) != hipSuccess)
            return fail(RV_E_DEVICE);
    }
    wit_count(w, cc.n_in + cc.n_in64 * 8);
    s->z64f = v.z64f;
    s->overlap = v.overlap;
    ctx->phase(RV_PH_SETUP);
    ctx->count();
    // (unrecorded proofs: the player keys come out of the one key-setup launch of shard_setup_prg)
    s->keys_deferred = !g_recorder && s->R == 4 * s->NQ;
    if (!s->keys_deferred) launch_expand_seeds(ctx->stream, s->d_seeds, s->R, s->d_keys);
    g_ht.mark("inputs");
    if ((rc = shard_setup_prg(s, nullptr))) return fail(rc);
    g_ht.mark("prg");
    prove_counted(PS_CALLS), prove_counted(PS_STAGE_IN, v.stage_in), prove_counted(PS_VCLR, v.vclr), prove_counted(PS_Z64F, s->z64f);
    prove_counted(PS_OVERLAP, s->overlap), prove_counted(PS_COL4, s->d_rk_c4 != nullptr);
    if (ec) s->ec = ec;  // (the caller made sure this path is taken)
    InterpParams p{};
    p.wit = s->d_wit;
    Interp64Params p64{};
    p64.wit = s->d_wit64;
    if (v.vclr) {
        if ((rc = dalloc(ctx, (size_t)cc.n_rows, &s->d_vclr))) return fail(rc);
        // (the zero row's value is cleared by k_shard_init: shard_run_alloc)
        p.vclr = s->d_vclr;
    }
    if ((rc = shard_run(s, v.vclr ? MODE_PROVE_V : MODE_PROVE, p, p64))) return fail(rc);
    if ((rc = shard_join(s))) return fail(rc);
    if (defer_sync) {
        ctx->prof.calls++;
        *out = s;
        return RV_OK;
    }
    int err = 0;
    if (hipMemcpyAsync(&err, s->d_err, sizeof err, hipMemcpyDeviceToHost, ctx->stream) != hipSuccess) return fail(RV_E_DEVICE);
    hipError_t e = hipStreamSynchronize(ctx->stream);
    if (e != hipSuccess) {
        hip_fail(e, "hipStreamSynchronize", __FILE__, __LINE__);
        return fail(RV_E_DEVICE);
    }
    ctx->collect();
    ctx->prof.calls++;
    if (err) return fail(RV_E_WITNESS_INVALID);
    *out = s;
    return RV_OK;
}

extern "C" int rv_shard_commit(rv_ctx* ctx, const rv_circuit* c, const uint8_t* wit_gf2, size_t n_gf2, const uint64_t* wit_z64,
                               size_t n_z64, const uint8_t* seeds, uint32_t rep_begin, uint32_t rep_count, rv_shard** out) {
    return guarded([&] { return rv_shard_commit_impl(ctx, c, wit_host(wit_gf2, n_gf2, wit_z64, n_z64), seeds, rep_begin, rep_count, out); });
}

// (RV_BATCH_STATS: when the calling thread's last plain-path proof had its commitment queued, its openings queued, its stream done -- ms since entry)
static thread_local double g_prove_marks[3];

// One call of rv_prove_impl, on its stack: run() takes the steps in order, each RV_OK or the call's code, and leaves through
// one exit that destroys the shard and frees a buffer nobody owns.  Owns the shard and -- unless the caller gave `dst` or the
// proof was handed over -- the proof's buffer.
//
// Early corrections (open.hip): half of a large GF(2) proof -- the corrections vectors -- does not depend on the
// challenge beyond the choice of repetitions.  Every repetition's vector goes to a page-locked staging buffer through
// the copy engine while the interpreter and the hash kernels run; once the challenge is known (published into a mapped
// mailbox the host polls, no stream synchronisation) helper threads copy the 40 opened ones into the proof while the GPU
// extracts the other half, which a kernel then writes around them into the same buffer.  RV_EARLY=0 turns it off.
//
// The plain path: commitment, challenge and openings all on the device (k_fs_challenge); the whole proof is laid out there
// in its final bincode form (comm included) and leaves in ONE copy; the host waits for the device once.
struct ProveRun {
    rv_ctx* ctx;
    const rv_circuit* c;
    const WitSrc& w;
    const uint8_t* seeds;
    uint8_t* dst;  // (nullable) the caller's page-locked buffer of dst_cap bytes (rv_prove_batch hands every proof a slice of one)
    size_t dst_cap;
    bool allow_early;

    uint8_t drawn[RV_TOTAL_REPS * RV_KEY_SIZE];
    ProveSchedule sch{};
    OpenLayout L{};  // of the whole framed proof
    EarlyRun er;
    rv_shard* s = nullptr;
    uint8_t* out = nullptr;        // the proof on the host
    uint8_t* out_dev = nullptr;    // early: its device address
    uint32_t* fs_dev = nullptr;    // early: the mailbox's
    uint8_t* stage_dev = nullptr;  // plain, small: the mapped staging buffer's
    OpenResult opened;
    uint32_t open_rep[RV_ONLINE_REPS], n_open = 0;  // early: the opened repetitions, from the mailbox

    // RV_EARLY_STATS (tools/early_ab.py reads the lines), g_prove_marks, g_ht (tools/batch_tail.py): ms since the call began
    struct Timing {
        const bool stats = getenv("RV_EARLY_STATS") && atoi(getenv("RV_EARLY_STATS"));
        const std::chrono::steady_clock::time_point t_begin = std::chrono::steady_clock::now();
        double t0 = 0, queued = 0, chal = 0, chunks = 0, copied = 0, sync = 0;
        double since() const { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_begin).count(); }
        void print_early() const {
            if (!stats) return;
            fprintf(stderr, "early: queued %.3f  challenge %.3f  chunks %.3f  copied %.3f  stream done %.3f ms", queued, chal, chunks, copied, sync);
            for (auto& m : g_ht.marks) fprintf(stderr, "  [%s %.3f]", m.first, m.second + t0);  // (RV_BATCH_STATS=1: the host's own marks)
            fprintf(stderr, "\n");
        }
    } t;

    int run(uint8_t** proof, size_t* proof_len) {
        const int rc = steps(proof, proof_len);
        if (!s) return rc;  // (nothing was queued)
        const double t_before_destroy = t.since();
        rv_shard_destroy(s);  // (waits for both streams: nothing writes into `out` any more)
        if (!dst) rv_free(out);
        if (t.stats) fprintf(stderr, "early: shard released %.3f -> %.3f ms\n", t_before_destroy, t.since());
        return rc;
    }
    int steps(uint8_t** proof, size_t* proof_len) {
        int rc;
        if ((rc = draw_seeds()) || (rc = arm_early()) || (rc = commit()) || (rc = proof_buffer())) return rc;
        if (sch.early) {
            if ((rc = open_early()) || (rc = copy_gaps()) || (rc = pump()) || (rc = await_challenge()) || (rc = gather_staged()) || (rc = settle())) return rc;
        } else if ((rc = map_stage_out()) || (rc = open()) || (rc = fetch())) {
            return rc;
        }
        return frame(proof, proof_len);
    }

    int draw_seeds() {
        if (seeds) return RV_OK;
        seeds = drawn;
        return os_seeds(drawn, sizeof drawn);
    }
    // the schedule; for an early proof the context's staging blocks, mailbox and helper threads, and the proof's sequence number
    int arm_early() {
        HIPCHK(hipSetDevice(ctx->device));
        sch = prove_schedule(ctx, c, RV_TOTAL_REPS, /*defer_sync=*/true, /*host_proof=*/true, allow_early && !dst);
        L = whole_proof_layout(c->cc);
        if (!sch.early) return RV_OK;
        const bool ok = ctx_stream2(ctx) == RV_OK && ctx->early_blocks(sch.plan->bytes, !sch.plan->z64, &fs_dev);
        if (!ok) {
            (void)hipGetLastError();
            plain_instead();
            return RV_OK;
        }
        if (!ctx->ec_pool) {
            constexpr int n_helpers = 9;
            ctx->ec_pool = new HelperPool(n_helpers);
        }
        // (test knob: the staging buffer starts every proof as garbage, so that bytes copied out of it before they arrived show)
        if (getenv("RV_EARLY_POISON") && atoi(getenv("RV_EARLY_POISON"))) memset(ctx->h_ec, 0x5A, sch.plan->bytes);
        er.plan = sch.plan;
        er.h_ec = ctx->h_ec;
        er.d_ec = ctx->d_ec;
        er.box_dev = fs_dev;
        er.box = ctx->h_fs;
        ctx->fs_seq = (ctx->fs_seq + 1) & 0xFFFFFFu;  // a fresh number even after a proof that failed half-way: its stamps must never match
        if (!ctx->fs_seq) ctx->fs_seq = 1;
        er.seq = ctx->fs_seq;
        return RV_OK;
    }
    void plain_instead() {
        sch.early = sch.early_z64 = false;
        sch.od = OpenDirect();
        sch.stage_out = L.total + 64 <= rv_ctx::STAGE_BYTES;
    }
    int commit() {
        t.t0 = t.since();  // when the commit phase began
        g_ht.begin();
        const int rc = rv_shard_commit_impl(ctx, c, w, seeds, 0, RV_TOTAL_REPS, &s, /*defer_sync=*/true, sch.early ? &er : nullptr, &sch);
        g_ht.mark("commit");
        if (!rc) g_prove_marks[0] = t.since();
        return rc;
    }
    // early: the proof's buffer, now that the GPU is busy (a fresh page-locked buffer of a 640 MB proof takes 45 ms to map).  Without
    // it the plain path still works: the stamps in the stream are harmless, nothing was handed to the second stream yet
    int proof_buffer() {
        if (sch.early && (!(out = (uint8_t*)out_alloc(L.total)) || hipHostGetDevicePointer((void**)&out_dev, out, 0) != hipSuccess || ((uintptr_t)out_dev & 15))) {
            (void)hipGetLastError();
            rv_free(out);
            out = nullptr;
            plain_instead();
            s->ec = nullptr;
        }
        prove_counted(PS_EARLY, sch.early), prove_counted(PS_EARLY_Z64, sch.early_z64), prove_counted(PS_OPEN_DIRECT, sch.od.n_direct != 0);
        return RV_OK;
    }
    // (the corrections vectors of the repetitions below r_spec are staged: the openings leave them out)
    int open_early() {
        if (sch.od.n_direct) s->od_out = out_dev, s->od_n_direct = sch.od.n_direct;
        OpenArgs a;
        a.framed = true;
        a.no_sync = true;
        a.fs_mailbox = fs_dev;
        a.fs_seq = er.seq;
        a.corr2_rep_min = sch.early_z64 ? 0 : er.plan->r_spec;
        a.corr64_rep_min = sch.early_z64 ? er.plan->r_spec : 0;
        if (int rc = shard_open_impl(s, a, &opened)) return rc;
        return opened.framed_total() != L.total || er.next != er.plan->chunks.size() || er.plan->chunks.size() > 255 ? RV_E_DEVICE : RV_OK;
    }
    // where the staged vectors go in the image: record j of their domain starts at rec_first + j * rec_size, its vector corr_at into it
    uint64_t corr_at() const { return 145 + (sch.early_z64 ? L.l64r : L.l2r); }
    uint64_t rec_first() const { return sch.early_z64 ? L.base[2] : L.base[0]; }
    uint64_t rec_size() const { return sch.early_z64 ? L.sz64 : L.sz2; }
    // the image without the corrections vectors, then the error word (mailbox word 8) in the same launch
    // (Z64: only the records of the opened repetitions below r_spec -- the kernel counts them -- go without their vectors)
    int copy_gaps() {
        launch_copy_gaps(ctx->stream, (const uint8_t*)opened.d, out_dev, L.total, rec_first(), rec_size(), corr_at(), sch.early_z64 ? L.l64c : L.l2c, RV_ONLINE_REPS,
                         s->d_omit, er.plan->r_spec, sch.od, s->d_err, (int*)(fs_dev + 8));
        if (hipGetLastError() != hipSuccess) return RV_E_DEVICE;
        t.queued = t.since();
        return RV_OK;
    }
    int pump() { return early_pump(s); }
    // the challenge: poll the mailbox (now and then make sure the stream is still alive)
    int await_challenge() {
        volatile uint32_t* box = ctx->h_fs;
        const uint32_t seq = er.seq;
        if (int rc = mailbox_wait(ctx, [&] { return __atomic_load_n(&box[0], __ATOMIC_ACQUIRE) == seq; }, &ctx->ec_wait_us[16], "early corrections (challenge)")) return rc;
        t.chal = t.since();
        const uint8_t* omit_all = (const uint8_t*)(ctx->h_fs + 16) + 32;
        for (uint32_t r = 0; r < RV_TOTAL_REPS; r++)
            if (omit_all[r] < RV_PLAYERS && n_open < RV_ONLINE_REPS) open_rep[n_open++] = r;
        return RV_OK;
    }
    // the copies of the chunks: normally long done; the host waits for the second stream (its copies complete in order), then every
    // thread (this one included) claims (chunk, opened repetition) pieces from one counter: a helper that wakes up late takes fewer
    // pieces instead of holding its share back
    int gather_staged() {
        if (hipStreamSynchronize(ctx->stream2) != hipSuccess) return hip_fail(hipGetLastError(), "early corrections (copies)", __FILE__, __LINE__);
        t.chunks = t.since();
        const auto& chunks = er.plan->chunks;
        const bool z64 = sch.early_z64;
        std::atomic<size_t> next_piece{0};
        // (Z64: the staging buffer holds the first r_spec repetitions; the opened ones among them are the first n_staged ranks)
        uint32_t n_staged = 0;
        for (uint32_t j = 0; j < n_open; j++)
            if (open_rep[j] < er.plan->r_spec) n_staged = j + 1;
        const size_t n_pieces = chunks.size() * n_staged;
        uint8_t* const first = out + rec_first() + corr_at();
        const size_t pitch = rec_size();
        const std::function<void(int)> job = [&](int) {
            for (;;) {
                const size_t piece = next_piece.fetch_add(1, std::memory_order_relaxed);
                if (piece >= n_pieces) return;
                const size_t j = piece % n_staged;
                const auto& ch = chunks[piece / n_staged];
                memcpy(first + j * pitch + ch.byte0, er.h_ec + ch.off + (size_t)open_rep[j] * ch.pitch + (z64 ? ch.byte0 : 0), ch.nbytes);
            }
        };
        ctx->ec_pool->run(job);
        t.copied = t.since();
        return RV_OK;
    }
    int settle() {
        if (hipStreamSynchronize(ctx->stream) != hipSuccess) return hip_fail(hipGetLastError(), "proof (early corrections)", __FILE__, __LINE__);
        t.sync = t.since();
        t.print_early();
        ctx->collect();
        if (n_open != RV_ONLINE_REPS) return RV_E_DEVICE;
        return (int)ctx->h_fs[8] ? RV_E_WITNESS_INVALID : RV_OK;
    }

    // small proofs: straight into the context's mapped staging buffer; the openings' launch may carry the error word there too
    int map_stage_out() {
        if (sch.stage_out) stage_dev = ctx->stage_mapped();
        sch.stage_out = stage_dev != nullptr;
        prove_counted(PS_STAGE_OUT, sch.stage_out);
        if (stage_dev) s->err_dst_mapped = (int*)(stage_dev + err_at());
        return RV_OK;
    }
    size_t err_at() const { return (L.total + 15) & ~(size_t)15; }
    int open() {
        OpenArgs a;
        a.dst = stage_dev;
        a.framed = true;
        a.no_sync = true;
        if (int rc = shard_open_impl(s, a, &opened)) return rc;
        if (dst && opened.framed_total() > dst_cap) return RV_E_ARG;
        out = dst ? dst : (uint8_t*)out_alloc(opened.framed_total());
        if (!out) return RV_E_NOMEM;
        g_ht.mark("open");
        g_prove_marks[1] = t.since();
        return RV_OK;
    }
    int fetch() {
        const size_t total = opened.framed_total();
        int err = 0;
        if (stage_dev) {
            if (total != L.total) return RV_E_DEVICE;
            if (!s->err_word_sent) launch_store_word(ctx->stream, s->d_err, (int*)(stage_dev + err_at()));
            if (hipStreamSynchronize(ctx->stream) != hipSuccess) return hip_fail(hipGetLastError(), "proof (staged)", __FILE__, __LINE__);
            memcpy(&err, ctx->h_stage + err_at(), sizeof err);
            memcpy(out, ctx->h_stage, total);
        } else if (hipMemcpyAsync(out, opened.d, total, hipMemcpyDeviceToHost, ctx->stream) != hipSuccess ||
                   hipMemcpyAsync(&err, s->d_err, sizeof err, hipMemcpyDeviceToHost, ctx->stream) != hipSuccess ||
                   hipStreamSynchronize(ctx->stream) != hipSuccess) {
            return hip_fail(hipGetLastError(), "proof D2H", __FILE__, __LINE__);
        }
        g_prove_marks[2] = t.since();
        ctx->collect();
        return err ? RV_E_WITNESS_INVALID : RV_OK;
    }

    // the shared tail: the four repetition counts, the proof handed over
    int frame(uint8_t** proof, size_t* proof_len) {
        frame_counts_host(out, opened.lens);
        *proof = out;
        *proof_len = opened.framed_total();
        out = nullptr;
        if (sch.early) g_early_proofs.fetch_add(1, std::memory_order_relaxed);
        if (sch.od.n_direct) g_open_direct_proofs.fetch_add(1, std::memory_order_relaxed);
        return RV_OK;
    }
};

// dst (nullable): page-locked destination of at least dst_cap bytes supplied by the caller; otherwise the proof gets a buffer of
// its own.  allow_early: the early-corrections path may be taken (prove_schedule)
static int rv_prove_impl(rv_ctx* ctx, const rv_circuit* c, const WitSrc& w, const uint8_t* seeds, uint8_t** proof, size_t* proof_len, uint8_t* dst = nullptr,
                         size_t dst_cap = 0, bool allow_early = true) {
    LibBusy busy_guard;  // (compile.h: the background unmapper keeps still while the GPU is driven)
    if (!ctx || !c || !proof || !proof_len) return RV_E_ARG;
    *proof = nullptr;
    *proof_len = 0;
    ProveRun run{ctx, c, w, seeds, dst, dst_cap, allow_early};
    return run.run(proof, proof_len);
}

extern "C" int rv_prove(rv_ctx* ctx, const rv_circuit* c, const uint8_t* wit_gf2, size_t n_gf2, const uint64_t* wit_z64,
                        size_t n_z64, const uint8_t* seeds, uint8_t** proof, size_t* proof_len) {
    return guarded([&] { return rv_prove_impl(ctx, c, wit_host(wit_gf2, n_gf2, wit_z64, n_z64), seeds, proof, proof_len); });
}

// A whole proof committed, opened with device Fiat-Shamir into the caller's device memory, the error word fetched: one
// synchronisation.  framed: the framing of a whole Proof around the sections, the repetition counts from k_frame_counts;
// otherwise the four sections alone, and omit and comm come back to the host with the error word.  lens (nullable): the sections'
static int prove_whole_to_device(rv_ctx* ctx, const rv_circuit* c, const WitSrc& w, const uint8_t* seeds, void* d_dst, bool framed, uint8_t* comm,
                                 uint8_t* omit, size_t* lens, const char* what) {
    rv_shard* s = nullptr;
    int rc = rv_shard_commit_impl(ctx, c, w, seeds, 0, RV_TOTAL_REPS, &s, /*defer_sync=*/true);
    if (rc) return rc;
    rc = [&]() -> int {
        OpenArgs a;
        a.dst = d_dst;
        a.framed = framed;
        a.no_sync = true;
        OpenResult res;
        if (int ro = shard_open_impl(s, a, &res)) return ro;
        for (int k = 0; k < 4 && lens; k++) lens[k] = res.lens[k];
        if (framed && (!launch_frame_counts(ctx->stream, (uint8_t*)d_dst, 0, 1, res.lens) || hipGetLastError() != hipSuccess)) return RV_E_DEVICE;
        uint8_t back[RV_TOTAL_REPS + 32];  // omit of the (whole) shard, then comm
        int err = 0;
        if ((!framed && hipMemcpyAsync(back, s->d_omit, sizeof back, hipMemcpyDeviceToHost, ctx->stream) != hipSuccess) ||
            hipMemcpyAsync(&err, s->d_err, sizeof err, hipMemcpyDeviceToHost, ctx->stream) != hipSuccess || hipStreamSynchronize(ctx->stream) != hipSuccess)
            return hip_fail(hipGetLastError(), what, __FILE__, __LINE__);
        ctx->collect();
        if (err) return RV_E_WITNESS_INVALID;
        if (!framed) {
            memcpy(omit, back, RV_TOTAL_REPS);
            memcpy(comm, back + RV_TOTAL_REPS, 32);
        }
        return RV_OK;
    }();
    rv_shard_destroy(s);
    return rc;
}

static int rv_prove_device_impl(rv_ctx* ctx, const rv_circuit* c, const WitSrc& w, const uint8_t* seeds, void* dst_device, uint8_t comm[RV_HASH_SIZE],
                                uint8_t omit[RV_TOTAL_REPS], size_t lens[4]) {
    LibBusy busy_guard;  // (compile.h: the background unmapper keeps still while the GPU is driven)
    if (!ctx || !c || !seeds || !dst_device || !comm || !omit || !lens) return RV_E_ARG;
    return prove_whole_to_device(ctx, c, w, seeds, dst_device, /*framed=*/false, comm, omit, lens, "rv_prove_device");
}

extern "C" int rv_prove_device(rv_ctx* ctx, const rv_circuit* c, const uint8_t* wit_gf2, size_t n_gf2, const uint64_t* wit_z64,
                               size_t n_z64, const uint8_t* seeds, void* dst_device, uint8_t comm[RV_HASH_SIZE],
                               uint8_t omit[RV_TOTAL_REPS], size_t lens[4]) {
    return guarded([&] { return rv_prove_device_impl(ctx, c, wit_host(wit_gf2, n_gf2, wit_z64, n_z64), seeds, dst_device, comm, omit, lens); });
}
