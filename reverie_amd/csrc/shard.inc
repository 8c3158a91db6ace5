// RV_BATCH_STATS: where the HOST's time goes while a proof is queued (thread-local; rv_prove_batch prints the marks of slow proofs)
struct HostTrace {
    bool on = false;
    std::chrono::steady_clock::time_point t0;
    std::vector<std::pair<const char*, double>> marks;
    void begin() {
        static const bool env = getenv("RV_BATCH_STATS") != nullptr;
        on = env;
        marks.clear();
        t0 = std::chrono::steady_clock::now();
    }
    void mark(const char* what) {
        if (on) marks.emplace_back(what, std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count());
    }
};
static thread_local HostTrace g_ht;

// n bytes of seed material from the OS, where the reference uses OsRng (proof/mod.rs:131-134)
static int os_seeds(uint8_t* buf, size_t n) {
    for (size_t got = 0; got < n;) {
        const ssize_t k = getrandom(buf + got, n - got, 0);
        if (k <= 0) return RV_E_DEVICE;
        got += (size_t)k;
    }
    return RV_OK;
}
// Part of api.hip (#included there, one translation unit): the shard: per-proof device state, the early-corrections plan, the mask generator beside the levels, the level loop, digests, commitment.

// ------------------------------------------------------------------------------------
// shard
// ------------------------------------------------------------------------------------
// one proof's early corrections: the plan, the device / host staging blocks, the chunks queued so far and the events that
// say a chunk has arrived on the host (owned by the shard's misc_events)
struct EarlyRun {
    const EarlyPlan* plan = nullptr;
    uint8_t* d_ec = nullptr;
    uint8_t* h_ec = nullptr;
    size_t next = 0;                 // chunks whose "ready" stamp is in the interpreter's stream
    size_t pumped = 0;               // chunks whose copy has been handed to the second stream
    // progress stamps in the context's host-mapped mailbox (no HIP events: their status reached the host late, and the
    // host must see a chunk the moment it is ready): word 1 = (seq << 8 | chunks ready)
    uint32_t* box_dev = nullptr;
    volatile uint32_t* box = nullptr;
    uint32_t seq = 0;
    bool ready(size_t k) const {
        const uint32_t v = __atomic_load_n(&box[1], __ATOMIC_ACQUIRE);
        return (v >> 8) == (seq & 0xFFFFFFu) && (v & 0xFFu) > k;
    }
};

struct rv_shard {
    rv_ctx* ctx = nullptr;
    const rv_circuit* c = nullptr;
    uint32_t rep_begin = 0, R = 0, NQ = 0;
    const uint32_t* d_on_quads = nullptr;  // verifier: the quad words that hold an opened repetition (not owned)
    uint32_t n_on_quads = 0;
    uint8_t* d_seeds = nullptr;
    uint8_t* d_keys = nullptr;
    uint8_t* d_rkbytes = nullptr;
    uint32_t* d_rk = nullptr;
    uint32_t* d_masks = nullptr;  // share rows: PRG masks, then computed rows
    uint32_t* d_rk_c4 = nullptr;  // the lane-distributed generator's key image (aes_col4.hip), when it is the one that runs
    // RV_OVERLAP: the generator runs chunk by chunk on ctx->stream_m BESIDE the level launches; a chunk is submitted (and its event
    // waited for on the main stream) right before the first level that reads it -- see overlap_need()
    bool overlap = false;
    uint64_t ov_head = 0;  // ... after the first ov_head CTR blocks, which the 128-plane generator writes before the first level (the verifier)
    uint64_t ov_next = 0, ov_blocks = 0, ov_chunk = 0;  // next block to generate, all of them, blocks per chunk
    const uint32_t* ov_keep = nullptr;
    uint8_t* d_wires = nullptr;   // corr bits [n_ssa][NQ/2]
    uint32_t* d_on = nullptr;
    uint8_t* d_pre = nullptr;     // [n_pre][NQ/2]
    uint8_t* d_wit = nullptr;
    uint8_t* d_vclr = nullptr;  // MODE_PROVE_V: cleartext value per share row
    // Z64 domain
    uint64_t* d_masks64 = nullptr;
    uint64_t* d_wmask64 = nullptr;
    uint64_t* d_wcorr64 = nullptr;
    bool z64f = false;            // the fused Z64 prover / verifier (internal.h: Z64FParams)
    hipEvent_t ev_sup64 = nullptr;        // ... set: the Z64 supplied values arrive on the side stream -- quad groups without an opened repetition run first
    std::function<int()> mid64;           // ... what brings them (the proof's copy, the unpack kernels), called once those groups' levels are queued
    const uint32_t* d_keep64z = nullptr;  // ... the verifier's kept streams per quad word (inside a block the caller tracks)
    uint64_t* d_v64 = nullptr;    // ... its cleartext values, one per Z64 SSA id
    uint64_t* d_on64 = nullptr;
    uint64_t* d_pre64 = nullptr;
    uint64_t* d_wit64 = nullptr;
    uint8_t* d_keys64 = nullptr;  // verifier only: the z64 openings carry their own key set
    uint32_t* d_rk64 = nullptr;
    uint8_t* d_omit64 = nullptr;
    uint32_t* d_cv[2] = {nullptr, nullptr};
    uint32_t* d_cv2[2] = {nullptr, nullptr};  // the online stream's pair when the two GF(2) trees share their launches (launch_b3_pair_big; owned through `extra`)
    uint32_t* d_dig = nullptr;  // [4][R][8]: pre2, on2, pre64, on64
    uint8_t* d_h = nullptr;     // [R][32]
    int* d_err = nullptr;
    // open
    uint8_t* d_omit = nullptr;
    uint64_t* d_offs = nullptr;  // [5][R]
    uint8_t* d_out = nullptr;
    std::vector<void*> extra;
    // pipelining: the gf2 mask generator runs in chunks on ctx->stream; the interpreter (on
    // ctx->stream2) waits for the chunk a level needs
    std::vector<std::pair<uint64_t, hipEvent_t>> mask_chunks;  // (AES blocks complete, event)
    hipEvent_t ev_setup = nullptr;
    std::vector<hipEvent_t> misc_events;
    struct EarlyRun* ec = nullptr;  // early corrections of this proof (not owned)
    // rv_prove's early path (internal.h: OpenDirect): the page-locked proof buffer's device address and the share of the broadcast
    // vectors' tiles that the extraction kernel writes there itself
    uint8_t* od_out = nullptr;
    uint32_t od_n_direct = 0;
    // small proofs (open.hip: k_open_small): where the openings' one launch also leaves the error word for the host, and whether it did
    int* err_dst_mapped = nullptr;
    bool err_word_sent = false;
    bool keys_deferred = false;  // rv_shard_commit: expand_seeds is part of shard_setup_prg's k_setup_keys
    bool dig64_filled = false;  // the empty Z64 transcripts' digests were written by k_shard_init

    void destroy() {
        for (auto& c : mask_chunks) ctx->sync_pool.push_back(c.second);
        mask_chunks.clear();
        for (hipEvent_t e : misc_events) ctx->sync_pool.push_back(e);
        misc_events.clear();
        if (ev_setup) ctx->sync_pool.push_back(ev_setup);
        ev_setup = nullptr;
        void* ps[] = {d_seeds, d_keys, d_rkbytes, d_rk,    d_masks,  d_wires,   d_on,     d_pre,    d_wit,  d_cv[0],
                      d_cv[1], d_dig,  d_h,       d_err,   d_omit,   d_offs,    d_out,    d_masks64, d_wmask64,
                      d_wcorr64, d_on64, d_pre64, d_wit64, d_keys64, d_rk64,    d_omit64, d_vclr, d_v64, d_rk_c4};
        for (void* p : ps) ctx->release(p);
        for (void* p : extra) ctx->release(p);
    }
};

extern "C" void rv_shard_destroy(rv_shard* s) {
    if (!s) return;
    (void)hipStreamSynchronize(s->ctx->stream);
    // work forked onto the second stream (the verifier's side copy of the proof, the two-stream pipeline): its buffers go back to
    // the arena below and the caller's host buffers leave scope -- nothing of it may still be in flight
    if (s->ctx->stream2 && (!s->misc_events.empty() || !s->mask_chunks.empty() || s->ev_setup || s->ec)) (void)hipStreamSynchronize(s->ctx->stream2);
    if (s->overlap && s->ctx->stream_m) (void)hipStreamSynchronize(s->ctx->stream_m);
    s->destroy();
    delete s;
}

struct OvTrace {  // RV_OV_TRACE=1: timing events around every chunk and every group of levels, printed by overlap_trace_dump
    std::vector<std::pair<std::string, hipEvent_t>> ev;
    void mark(const char* what, uint64_t n, hipStream_t st) {
        hipEvent_t e = nullptr;
        (void)hipEventCreate(&e);
        (void)hipEventRecord(e, st);
        ev.emplace_back(std::string(what) + " " + std::to_string(n), e);
    }
};
static thread_local OvTrace* g_ov_trace = nullptr;
static void overlap_trace_dump() {
    if (!g_ov_trace) return;
    for (auto& kv : g_ov_trace->ev) {
        float ms = 0;
        (void)hipEventSynchronize(kv.second);
        (void)hipEventElapsedTime(&ms, g_ov_trace->ev[0].second, kv.second);
        fprintf(stderr, "[ov] %9.1f us  %s\n", ms * 1e3, kv.first.c_str());
    }
    for (auto& kv : g_ov_trace->ev) (void)hipEventDestroy(kv.second);
    delete g_ov_trace;
    g_ov_trace = nullptr;
}
// Which GF(2) generator: the lane-distributed one (aes_col4.hip) whenever it is to share the chip with the level launches
// (RV_OVERLAP), for SMALL proofs (up to 4 096 cipher blocks per slot: the 128-plane kernel's wavefront runs 32 blocks per lane one
// round after the other, ~45 us however few there are; a quad of lanes per state is through in ~19 -- tools/gen_sweep.py: AES-128
// 0.27 -> 0.245 ms, even at 1 000 - 4 000 blocks, behind from 8 000), or on request (RV_AES_COL4=1 / 0, read once); recorded batches
// keep the 128-plane kernel (its launch is replayable)
static bool gf2_masks_col4(uint32_t NQ, uint64_t n_blocks, bool overlap) {
    static const int col4_mode = [] {
        const char* e = getenv("RV_AES_COL4");
        return e ? atoi(e) : -1;
    }();
    return n_blocks && !g_recorder && aes_col4_supports(NQ) && (col4_mode > 0 || (col4_mode < 0 && (overlap || n_blocks <= 4096)));
}
// key material -> bitsliced round keys, masks
static int shard_setup_prg(rv_shard* s, const uint32_t* d_keep, const uint32_t* d_keep64 = nullptr) {
    rv_ctx* ctx = s->ctx;
    const Compiled& cc = s->c->cc;
    int rc;
    const uint64_t n_blocks64 = (cc.n_masks64 + 1) / 2;
    if (n_blocks64) {
        if ((rc = dalloc(ctx, (size_t)n_blocks64 * 2 * s->R * 8, &s->d_masks64))) return rc;
        if (s->d_keys64) {  // verifier: separate key set for the z64 transcript (reuses d_rkbytes as scratch below)
            if ((rc = dalloc(ctx, (size_t)RK_AREAS * 128 * s->NQ, &s->d_rk64))) return rc;
        }
    }
    if ((rc = dalloc(ctx, (size_t)s->R * 8 * RK_BYTES, &s->d_rkbytes))) return rc;
    if ((rc = dalloc(ctx, (size_t)RK_AREAS * 128 * s->NQ, &s->d_rk))) return rc;
    const uint64_t n_blocks = cc.n_masks_pad / 128;
    if ((rc = dalloc(ctx, (size_t)cc.n_rows * s->NQ, &s->d_masks))) return rc;
    if (!s->keys_deferred) {
        launch_key_schedule(ctx->stream, s->d_keys, s->R * 8, s->d_rkbytes);
        launch_bitslice_rk(ctx->stream, s->d_rkbytes, s->NQ, s->d_rk);
        ctx->count(2);
    }
    const bool col4 = gf2_masks_col4(s->NQ, n_blocks, s->overlap);
    if (s->overlap && !col4) s->overlap = false;
    if (col4) {
        if ((rc = dalloc(ctx, aes_col4_image_bytes(s->NQ) / 4, &s->d_rk_c4))) return rc;
        if (!s->keys_deferred) {
            launch_rk_col4(ctx->stream, s->d_rk, s->NQ, s->d_rk_c4);
            ctx->count();
        }
    }
    if (s->keys_deferred) {
        // (rv_shard_commit left the seeds' expansion to this launch: aes.hip, k_setup_keys)
        launch_setup_keys(ctx->stream, s->d_seeds, s->NQ, s->d_keys, s->d_rkbytes, s->d_rk, col4 ? s->d_rk_c4 : nullptr);
        ctx->count();
    }
    ctx->phase(RV_PH_MASKS);
    if (n_blocks64) {
        const uint32_t* rk64 = s->d_rk;  // prover: the same seeds feed both domains (proof/mod.rs:131-146)
        if (s->d_keys64) {
            launch_key_schedule(ctx->stream, s->d_keys64, s->R * 8, s->d_rkbytes);
            launch_bitslice_rk(ctx->stream, s->d_rkbytes, s->NQ, s->d_rk64);
            rk64 = s->d_rk64;
        }
        if (s->z64f) {
            // only the Input gates' rows: a Mul's two masks come out of the interpreter's own launches
            s->d_keep64z = s->d_keys64 ? d_keep64 : d_keep;
            for (const auto& run : s->c->z64f_runs) {
                launch_aes_z64_masks(ctx->stream, rk64, s->d_keep64z, s->NQ, run.second, s->d_masks64 + (size_t)run.first * 2 * s->R * 8, run.first);
                ctx->count(1);
            }
        } else {
            launch_aes_z64_masks(ctx->stream, rk64, s->d_keys64 ? d_keep64 : d_keep, s->NQ, n_blocks64, s->d_masks64);
            ctx->count(1);
        }
    }
    if (s->overlap) {
        // nothing is generated here: the level loop submits the chunks (overlap_need), each on ctx->stream_m behind this point
        if (!ctx->stream_m && (ctx->has_prio ? hipStreamCreateWithPriority(&ctx->stream_m, hipStreamNonBlocking, ctx->mask_prio)
                                             : hipStreamCreateWithFlags(&ctx->stream_m, hipStreamNonBlocking)) != hipSuccess)
            return hip_fail(hipGetLastError(), "hipStreamCreate", __FILE__, __LINE__);
        s->ev_setup = ctx->get_sync_event();
        HIPCHK(hipEventRecord(s->ev_setup, ctx->stream));
        HIPCHK(hipStreamWaitEvent(ctx->stream_m, s->ev_setup, 0));
        static const uint64_t n_chunks = [] {
            const char* e = getenv("RV_OVERLAP_CHUNKS");
            return (uint64_t)std::min(std::max(e ? atoi(e) : 16, 1), 256);
        }();
        s->ov_blocks = n_blocks;
        s->ov_chunk = std::max<uint64_t>((n_blocks + n_chunks - 1) / n_chunks, 1024);
        s->ov_keep = d_keep;
        // the verifier's levels cannot start before the proof has crossed PCIe and its supplied values are unpacked (1.2 ms for the
        // 50 MB proof): the stand-alone generator fills that window with the first ov_head blocks, only the rest runs beside the levels
        const uint64_t head = std::min(s->ov_head, n_blocks);
        if (head) {
            launch_aes_gf2_masks(ctx->stream, s->d_rk, d_keep, s->NQ, 0, head, s->d_masks);
            ctx->count();
            s->ov_next = head;
        }
        static const bool trace = getenv("RV_OV_TRACE") && atoi(getenv("RV_OV_TRACE")) != 0;
        if (trace) {
            overlap_trace_dump();  // (the previous proof's)
            g_ov_trace = new OvTrace();
            g_ov_trace->mark("main: keys done", 0, ctx->stream);
        }
        ctx->phase(-1);
        return RV_OK;
    }
    // every GF(2) mask before the first level, on the main stream
    if (n_blocks) {
        if (col4)
            launch_aes_gf2_masks_col4(ctx->stream, s->d_rk_c4, d_keep, s->NQ, 0, n_blocks, s->d_masks);
        else
            launch_aes_gf2_masks(ctx->stream, s->d_rk, d_keep, s->NQ, 0, n_blocks, s->d_masks);
        ctx->count();
    }
    ctx->phase(-1);
    return RV_OK;
}

// RV_OVERLAP: make sure the masks of CTR blocks [0, need) are on their way and ordered before what the main stream queues next.
// hipStreamWaitEvent orders behind the OTHER stream's tail at the time it is queued (DESIGN.md, runtime lessons of round 4), so a
// chunk is submitted right before the first level that reads it and waited for at once: the host runs far ahead of the device,
// every chunk sits in stream_m's queue long before its turn, and the generator runs back to back beside the levels.
static int overlap_need(rv_shard* s, uint64_t need, hipStream_t sb) {
    rv_ctx* ctx = s->ctx;
    need = std::min(need, s->ov_blocks);
    while (s->ov_next < need) {
        if (g_ov_trace) g_ov_trace->mark("main: levels queued so far end; wait for chunk ending at block", s->ov_next, sb);
        if (g_ov_trace) g_ov_trace->mark("  masks: chunk start at block", s->ov_next, ctx->stream_m);
        // (the first chunk is what the proof waits for with nothing beside it: half size)
        const uint64_t nb = std::min(s->ov_next == 0 ? std::max<uint64_t>(s->ov_chunk / 2, 512) : s->ov_chunk, s->ov_blocks - s->ov_next);
        const auto ht0 = std::chrono::steady_clock::now();
        launch_aes_gf2_masks_col4(ctx->stream_m, s->d_rk_c4, s->ov_keep, s->NQ, s->ov_next, nb, s->d_masks + (size_t)s->ov_next * 128 * s->NQ);
        const auto ht1 = std::chrono::steady_clock::now();
        ctx->count();
        s->ov_next += nb;
        hipEvent_t e = ctx->get_sync_event();
        HIPCHK(hipEventRecord(e, ctx->stream_m));
        const auto ht2 = std::chrono::steady_clock::now();
        s->mask_chunks.emplace_back(s->ov_next, e);
        if (g_ov_trace) g_ov_trace->mark("  masks: chunk end at block", s->ov_next, ctx->stream_m);
        HIPCHK(hipStreamWaitEvent(sb, e, 0));
        if (g_ht.on) {
            const auto ht3 = std::chrono::steady_clock::now();
            auto ms = [](std::chrono::steady_clock::time_point a, std::chrono::steady_clock::time_point b) { return std::chrono::duration<double, std::milli>(b - a).count(); };
            if (ms(ht0, ht1) > 2) g_ht.mark("(slow: chunk launch)");
            if (ms(ht1, ht2) > 2) g_ht.mark("(slow: chunk event record)");
            if (ms(ht2, ht3) > 2) g_ht.mark("(slow: wait event)");
        }
        if (g_ov_trace) g_ov_trace->mark("main: chunk arrived, levels go on; block", s->ov_next, sb);
    }
    return RV_OK;
}

// BLAKE3("") as eight words: the digest of an empty transcript
static const uint32_t* b3_empty_digest() {
    static const std::vector<uint32_t> empty = [] {
        b3::Hasher hs;
        uint8_t out[32];
        hs.finalize(out);
        std::vector<uint32_t> w(8);
        for (int k = 0; k < 8; k++) w[k] = (uint32_t)out[4 * k] | ((uint32_t)out[4 * k + 1] << 8) | ((uint32_t)out[4 * k + 2] << 16) | ((uint32_t)out[4 * k + 3] << 24);
        return w;
    }();
    return empty.data();
}

// The interpreter phase of a shard in three steps (shard_run = all three; rv_prove_batch interleaves them over several
// shards): buffers + parameter blocks, the level loop, the transcript digests.
static int shard_run_alloc(rv_shard* s, InterpParams& p, Interp64Params& p64) {
    rv_ctx* ctx = s->ctx;
    const Compiled& cc = s->c->cc;
    int rc;
    if ((rc = dalloc(ctx, (size_t)cc.n_rows * (s->NQ / 2), &s->d_wires))) return rc;  // corr bits per base row
    if ((rc = dalloc(ctx, (size_t)std::max<uint64_t>(cc.n_on, 1) * s->NQ, &s->d_on))) return rc;
    if ((rc = dalloc(ctx, (size_t)std::max<uint64_t>(cc.n_pre, 1) * (s->NQ / 2), &s->d_pre))) return rc;
    if (!s->d_err && (rc = dalloc(ctx, 1, &s->d_err))) return rc;  // (rv_prove_batch hands every proof a slot of one array)
    const size_t cvw = b3_stream_scratch_words(std::max({cc.n_on, cc.n_pre, cc.on_words64 * 8, cc.pre_words64 * 8}), s->R);
    if ((rc = dalloc(ctx, cvw, &s->d_cv[0])) || (rc = dalloc(ctx, cvw, &s->d_cv[1]))) return rc;
    if (b3_pair_big_ok(cc.n_pre, cc.n_on, s->NQ, s->d_on_quads, s->n_on_quads)) {  // (the two GF(2) trees in shared launches: buffers of their own for the second)
        const size_t w2 = b3_stream_scratch_words(std::max(cc.n_on, cc.n_pre), s->R);
        if ((rc = dalloc(ctx, w2, &s->d_cv2[0])) || (rc = dalloc(ctx, w2, &s->d_cv2[1]))) return rc;
        s->extra.push_back(s->d_cv2[0]);
        s->extra.push_back(s->d_cv2[1]);
    }
    if ((rc = dalloc(ctx, (size_t)4 * s->R * 8, &s->d_dig))) return rc;
    if (!s->d_h && (rc = dalloc(ctx, (size_t)s->R * 32, &s->d_h))) return rc;  // (rv_verify_batch: a slot of one array)
    const bool has64 = !cc.gates64.empty();
    if (has64) {
        if ((rc = dalloc(ctx, (size_t)cc.n_ssa64 * s->R * 8, &s->d_wmask64))) return rc;
        if (s->z64f && !s->d_keys64) {  // (the fused PROVER: cleartext values; the verifier keeps per-repetition corrections)
            if ((rc = dalloc(ctx, (size_t)cc.n_ssa64, &s->d_v64))) return rc;
            HIPCHK(hipMemsetAsync(s->d_v64, 0, 8, ctx->stream));  // (SSA id 0 = the zero wire; the fused path is never recorded)
        } else {
            if ((rc = dalloc(ctx, (size_t)cc.n_ssa64 * s->R, &s->d_wcorr64))) return rc;
            HIPCHK(rv::memset_async(s->d_wcorr64, 0, (size_t)s->R * 8, ctx->stream));  // (recorded by rv_prove_batch / rv_verify_batch)
        }
        if ((rc = dalloc(ctx, (size_t)std::max<uint64_t>(cc.on_words64, 1) * s->R, &s->d_on64))) return rc;
        if ((rc = dalloc(ctx, (size_t)std::max<uint64_t>(cc.pre_words64, 1) * s->R, &s->d_pre64))) return rc;
        HIPCHK(rv::memset_async(s->d_wmask64, 0, (size_t)s->R * 64, ctx->stream));
    }
    hipStream_t sb = ctx->stream;
    // error flag and the zero row (first computed row: mask 0, corr 0), one launch
    // (... and, for a pure GF(2) circuit, the digests of its two empty Z64 transcripts: shard_run_hash then has nothing to launch for them)
    s->dig64_filled = !g_recorder && cc.pre_words64 == 0 && cc.on_words64 == 0;
    launch_shard_init(sb, s->d_err, s->d_masks + (size_t)cc.zero_row * s->NQ, s->NQ,
                      s->d_wires + (size_t)cc.zero_row * (s->NQ / 2), s->NQ / 2, s->dig64_filled ? s->d_dig + 2 * (size_t)s->R * 8 : nullptr, 2 * s->R,
                      b3_empty_digest(), p.vclr ? p.vclr + cc.zero_row : nullptr);
    p.NQ = s->NQ;
    p.rows = s->d_masks;
    p.corr = s->d_wires;
    p.on = s->d_on;
    p.pre = s->d_pre;
    p.err = s->d_err;
    p64.R = s->R;
    p64.wmask = s->d_wmask64;
    p64.wcorr = s->d_wcorr64;
    p64.masks = s->d_masks64;
    p64.on = s->d_on64;
    p64.pre = s->d_pre64;
    p64.on_words = cc.on_words64;
    p64.pre_words = cc.pre_words64;
    p64.corr2 = s->d_wires;
    p64.masks2 = s->d_masks;
    p64.NQ = s->NQ;
    p64.err = s->d_err;
    return RV_OK;
}

// Batched proofs: an LDS run takes NQ / qs workgroups per proof, each alone on a compute unit and mostly waiting on its
// own dependency chain -- better than one workgroup per proof (k_interp_narrow_b, ~3x slower per proof) only while the
// whole batch still finds room on the chip at once or nearly so (RV_LDS_BATCH_WGS overrides the limit)
// one-quad slices update nibbles of the bit-packed rows through aligned 32-bit words: rows of at least four bytes (32 repetitions)
static bool lds_run_fits_rows(uint32_t qs, uint32_t NQ) { return NQ % qs == 0 && (qs > 1 || NQ % 8 == 0); }

static bool lds_run_for_batch(const rv_circuit* c, size_t level, size_t batch) {
    if (c->lds_run_of_level[level] < 0) return false;
    const auto& pl = c->lds_runs[(size_t)c->lds_run_of_level[level]];
    const size_t limit = getenv("RV_LDS_BATCH_WGS") ? (size_t)atoll(getenv("RV_LDS_BATCH_WGS")) : 768;
    return batch * (RV_TOTAL_REPS / 4 / pl.qs) <= limit;
}

// The early-corrections plan of a circuit: per level the smallest preprocessing row any LATER level still writes (a
// Mul's row number g.ep; everything below it is final), the corrections vector cut into RV_EARLY_CHUNKS (default 4:
// 4 and 5 give the same proof time, 3 and 6 .. 10 a longer one; every chunk costs a ~25 us packing kernel)
// byte ranges, each with the level it is complete after.  Only for pure GF(2) circuits with at least RV_EARLY_MIN
// (default 2^21) Mul gates whose preprocessing rows complete roughly in step with the levels (a layered circuit; a
// circuit whose first rows are written by its last level gains nothing and keeps the plain path).
static std::atomic<uint64_t> g_overlap_commits{0};  // shard commitments whose mask generator ran beside the level launches (RV_OVERLAP)
extern "C" uint64_t rv_hook_overlap_commits(void) { return g_overlap_commits.load(std::memory_order_relaxed); }
static std::atomic<uint64_t> g_early_proofs{0};
extern "C" uint64_t rv_hook_early_proofs(void) { return g_early_proofs.load(std::memory_order_relaxed); }
static std::atomic<uint64_t> g_open_direct_proofs{0};
extern "C" uint64_t rv_hook_open_direct_proofs(void) { return g_open_direct_proofs.load(std::memory_order_relaxed); }
// rv_hook_prove_schedule (prove.inc): what the single-proof prover's calls decided, cumulative, in the hook's order
enum { PS_CALLS, PS_EARLY, PS_EARLY_Z64, PS_OPEN_DIRECT, PS_STAGE_OUT, PS_STAGE_IN, PS_VCLR, PS_Z64F, PS_OVERLAP, PS_COL4,
       PS_OPEN_ONE, PS_OPEN_HEADS_INPUTS, PS_OPEN_SEPARATE, PS_OPEN_ERR_WORD, PS_N };
static std::atomic<uint64_t> g_prove_schedule[16];
static void prove_counted(int what, bool on = true) {
    if (on) g_prove_schedule[what].fetch_add(1, std::memory_order_relaxed);
}
static std::atomic<uint64_t> g_verify_vc{0};
extern "C" uint64_t rv_hook_verify_vc_count(void) { return g_verify_vc.load(std::memory_order_relaxed); }

// (the plan as the environment stands NOW: early_plan() below keeps the first one it builds for a circuit, rv_circuit_early_staging_bytes
// builds one of its own to answer with -- a query must not freeze the knobs the first proof would have read)
static void early_plan_build(const rv_circuit* c, EarlyPlan& P) {
    const Compiled& cc = c->cc;
    // (read per circuit, not once per process: the tests lower them)
    const uint64_t min_events = getenv("RV_EARLY_MIN") ? (uint64_t)atoll(getenv("RV_EARLY_MIN")) : (1ull << 21);
    // (the progress stamp carries the chunk count in eight bits; a bad knob gives no plan, i.e. the plain path, not a failed proof)
    const int n_chunks_env = getenv("RV_EARLY_CHUNKS") ? std::min(atoi(getenv("RV_EARLY_CHUNKS")), 255) : 4;
    auto reps_env = [](uint32_t dflt) -> uint32_t {
        const char* e = getenv("RV_EARLY_REPS");
        if (!e) return dflt;
        return (uint32_t)std::min(std::max(atoi(e), 0), (int)RV_TOTAL_REPS);
    };
    const size_t n_levels = cc.level_start.empty() ? 0 : cc.level_start.size() - 1;
    if (!cc.gates64.empty()) {
        // ---- Z64 ----
        const size_t n_lv64 = cc.level_start64.empty() ? 0 : cc.level_start64.size() - 1;
        const uint64_t min64 = getenv("RV_EARLY_MIN") ? min_events : (1ull << 17);
        if (cc.row_prg_base || cc.n_pre || cc.pre_words64 != cc.n_corr64 || cc.n_corr64 < min64 || (cc.n_corr64 & 1) || !n_lv64 || n_chunks_env < 1) return;
        std::vector<uint64_t> lo(n_lv64, UINT64_MAX);
        for (size_t l = 0; l < n_lv64; l++)
            for (uint32_t i = cc.level_start64[l]; i < cc.level_start64[l + 1]; i++) {
                const uint32_t op = cc.gates64[i].op;
                if (op == G64_B2A) return;
                if (op == G64_MUL) lo[l] = std::min<uint64_t>(lo[l], cc.gates64[i].ep);
            }
        std::vector<uint64_t> done(n_lv64);
        uint64_t m = cc.pre_words64;
        for (size_t l = n_lv64; l-- > 0;) {
            done[l] = m;
            m = std::min(m, lo[l]);
        }
        // how many repetitions' vectors fit through PCIe while the interpreter and the hashes run (rates of the 10^6-MUL
        // benchmark circuit: ~19 ns per gate, ~6 ns per Mul of hashing); RV_EARLY=2: RV_EARLY_REPS (default 128) whatever the estimate
        const uint64_t vec_bytes = 8 * cc.n_corr64;
        uint32_t r_spec;
        if (getenv("RV_EARLY") && atoi(getenv("RV_EARLY")) == 2) {
            r_spec = reps_env(128);
        } else {
            // (~19 ns per gate of interpreter + mask generator -- fused or not --, ~6 ns per Mul of hashing)
            const double t_window = (double)cc.gates64.size() * 19e-9 + (double)cc.n_corr64 * 6e-9;
            // 0.9 of what the window could carry.  Round 3 staged 128 repetitions of the benchmark circuit in FOUR chunks (more
            // made the proof slower: the last chunk, a quarter of everything, was still crossing PCIe at the challenge); in twelve
            // chunks the last one fits the hash phase and all 256 repetitions pay: 54.4 -> 52.7 (192) -> 51.8 ms (256), proofs of
            // both plans interleaved in one process (tools/z64_early_ab.py).  2 GB of page-locked staging instead of 1 GB.
            r_spec = (uint32_t)std::min<double>(RV_TOTAL_REPS, 0.9 * t_window * 55e9 / (double)vec_bytes);
        }
        r_spec = std::min<uint32_t>(r_spec, RV_TOTAL_REPS) & ~7u;
        if (r_spec < 64) return;
        const uint64_t pitch = (vec_bytes + 127) & ~127ull;
        const uint64_t K = getenv("RV_EARLY_CHUNKS") ? (uint64_t)n_chunks_env : 12;  // (Z64: twelve chunks unless told otherwise)
        const uint64_t per = ((vec_bytes + K - 1) / K + 127) & ~127ull;
        for (uint64_t b0 = 0; b0 < vec_bytes; b0 += per) {
            EarlyPlan::Chunk ch{};
            ch.byte0 = b0;
            ch.nbytes = std::min(per, vec_bytes - b0);
            ch.pitch = pitch;
            ch.off = 0;
            const uint64_t need = (ch.byte0 + ch.nbytes) / 8;
            ch.ready_level = (uint32_t)(std::lower_bound(done.begin(), done.end(), need) - done.begin());
            if (ch.ready_level >= n_lv64) return;
            const uint64_t k = P.chunks.size();
            if (ch.ready_level > n_lv64 * (k + 1) / K + n_lv64 / 4) return;
            P.chunks.push_back(ch);
        }
        P.bytes = (size_t)r_spec * pitch;
        P.z64 = true;
        P.r_spec = r_spec;
        P.ok = true;
        return;
    }
    if (cc.row_prg_base || cc.n_pre < min_events || !n_levels || n_chunks_env < 1) return;
    // The staged repetitions' vectors (1/8 byte per Mul each) must cross PCIe (~55 GB/s) while the interpreter and the hash kernels
    // run, or the copies pile up behind the challenge and the proof gets SLOWER (all 256 on the all-AND variant of the 10^7-gate
    // circuit, 320 MB against ~4.6 ms: 10.9 -> 11.0 - 11.6 ms).  So only as many repetitions as fit 0.9 of the estimated window
    // (the benchmark circuits' rates: a level launch >= 13 us and ~0.25 ns per gate, the hashes ~0.21 ns per Mul); the opened
    // repetitions beyond them are extracted and copied the plain way.  RV_EARLY=2: all of them (RV_EARLY_REPS overrides).
    uint32_t r_spec = RV_TOTAL_REPS;
    if (getenv("RV_EARLY") && atoi(getenv("RV_EARLY")) == 2) {
        r_spec = reps_env(RV_TOTAL_REPS);
    } else {
        // (round 6: since the mask generator runs BESIDE the levels (RV_OVERLAP) the phase is as long as the cipher needs, ~38 ns per CTR
        // block of 64 quad words -- 6.0 ms on the all-AND variant, where the old estimate staged 192 of the 256 repetitions and the proof
        // paid for the rest behind the challenge: 10.18 -> 9.64 ms with all of them)
        const bool beside = !(getenv("RV_OVERLAP") && atoi(getenv("RV_OVERLAP")) == 0);  // (with the masks BEFORE the first level the window is the levels' own time)
        const double t_levels = std::max({(double)n_levels * 13e-6, (double)cc.gates.size() * 0.25e-9, beside ? (double)(cc.n_masks_pad / 128) * 38e-9 : 0.0});
        const double t_window = t_levels + (double)cc.n_pre * 0.21e-9 + 0.3e-3;
        r_spec = (uint32_t)std::min<double>(RV_TOTAL_REPS, 0.9 * t_window * 55e9 / ((double)cc.n_pre / 8.0));
    }
    r_spec = std::min<uint32_t>(r_spec, RV_TOTAL_REPS) & ~7u;
    if (r_spec < 64) return;
    // smallest row written per level, on a few threads (10^7 gate records are 0.4 GB)
    std::vector<uint64_t> lo(n_levels, UINT64_MAX);
    const int T = std::max(1, std::min<int>(16, (int)std::thread::hardware_concurrency()));
    auto scan = [&](size_t l0, size_t l1) {
        for (size_t l = l0; l < l1; l++) {
            uint64_t m = UINT64_MAX;
            for (uint32_t i = cc.level_start[l]; i < cc.level_start[l + 1]; i++)
                if (g_op(cc.gates[i]) == G_MUL) m = std::min<uint64_t>(m, cc.gates[i].ep);
            lo[l] = m;
        }
    };
    {
        std::vector<std::thread> th;
        size_t l0 = 0;
        for (int t = 0; t < T; t++) {
            // levels dealt by gate count
            const uint32_t want = (uint32_t)((uint64_t)cc.gates.size() * (t + 1) / T);
            size_t l1 = t + 1 == T ? n_levels : (size_t)(std::lower_bound(cc.level_start.begin(), cc.level_start.end(), want) - cc.level_start.begin());
            l1 = std::min(std::max(l1, l0), n_levels);
            if (l1 > l0) {
                if (t + 1 == T) scan(l0, l1); else th.emplace_back(scan, l0, l1);
            }
            l0 = l1;
        }
        for (auto& t : th) t.join();
    }
    // done[l] = rows final once levels 0 .. l have run
    std::vector<uint64_t> done(n_levels);
    uint64_t m = cc.n_pre;
    for (size_t l = n_levels; l-- > 0;) {
        done[l] = m;
        m = std::min(m, lo[l]);
    }
    const uint64_t l2c = cc.n_pre / 8 + 1;
    const uint64_t K = (uint64_t)n_chunks_env;
    const uint64_t per = ((l2c + K - 1) / K + 127) & ~127ull;
    size_t off = 0;
    for (uint64_t b0 = 0; b0 < l2c; b0 += per) {
        EarlyPlan::Chunk ch{};
        ch.byte0 = b0;
        ch.nbytes = std::min(per, l2c - b0);
        ch.pitch = (ch.nbytes + 127) & ~127ull;
        ch.off = off;
        off += (size_t)256 * ch.pitch;
        const uint64_t need = std::min<uint64_t>(8 * (ch.byte0 + ch.nbytes), cc.n_pre);
        ch.ready_level = (uint32_t)(std::lower_bound(done.begin(), done.end(), need) - done.begin());
        if (ch.ready_level >= n_levels) return;  // (cannot happen: done[last] = n_pre)
        const uint64_t k = P.chunks.size();
        if (ch.ready_level > n_levels * (k + 1) / K + n_levels / 4) return;  // completes too late to be worth sending ahead
        P.chunks.push_back(ch);
    }
    P.bytes = off;
    P.r_spec = r_spec;
    P.ok = true;
}
static const EarlyPlan* early_plan(const rv_circuit* c) {
    std::call_once(c->ec_once, [c] { early_plan_build(c, c->ec_plan); });
    return &c->ec_plan;
}
static uint64_t early_staging_bytes_of(const rv_circuit* c) {
    if (const char* e = getenv("RV_EARLY"))
        if (atoi(e) == 0) return 0;
    EarlyPlan P;
    early_plan_build(c, P);
    return P.ok ? (uint64_t)P.bytes : 0;
}

// Host-only view of the plan (tests): compiles the ops as rv_circuit_compile_ex would, builds the early-corrections plan and checks
// it against the gate records one by one -- no gate of a level after a chunk's ready_level may write a preprocessing row of the chunk,
// and some gate of the ready_level itself must (else the chunk could have left a level earlier).  out[0] = plan taken (0 / 1),
// [1] = Z64 form, [2] = staged repetitions, [3] = chunks, [4] = staging bytes, [5] = the check (1 = consistent), [6 + k] = chunk k's
// ready_level (k < 16).
extern "C" int rv_hook_early_plan(const rv_op* ops, size_t n_ops, size_t z64_wires, size_t gf2_wires, uint32_t flags, uint64_t out[22]) {
    if (!out || (n_ops && !ops) || (flags & ~RV_COMPILE_WHOLE_PROVER)) return RV_E_ARG;
    return guarded([&]() -> int {
        rv_circuit tmp;
        int rc = compile_ops(ops, n_ops, z64_wires, gf2_wires, tmp.cc, nullptr, ((flags & RV_COMPILE_WHOLE_PROVER) && !getenv("RV_LAZY_K")) ? RV_LIN_K : 0);
        if (rc) return rc;
        const EarlyPlan* P = early_plan(&tmp);
        for (int i = 0; i < 22; i++) out[i] = 0;
        out[0] = P->ok, out[1] = P->z64, out[2] = P->r_spec, out[3] = P->chunks.size(), out[4] = P->bytes;
        if (!P->ok) return RV_OK;
        const Compiled& cc = tmp.cc;
        bool good = true;
        for (size_t k = 0; k < P->chunks.size(); k++) {
            const auto& ch = P->chunks[k];
            if (k < 16) out[6 + k] = ch.ready_level;
            // rows (GF(2): 8 per byte; Z64: one word per 8 bytes) of the chunk
            const uint64_t row0 = P->z64 ? ch.byte0 / 8 : ch.byte0 * 8;
            const uint64_t row1 = P->z64 ? (ch.byte0 + ch.nbytes) / 8 : std::min<uint64_t>((ch.byte0 + ch.nbytes) * 8, cc.n_pre);
            bool at_ready = row1 <= row0;  // (the pad byte behind the last row belongs to no gate)
            const size_t n_levels = (P->z64 ? cc.level_start64.size() : cc.level_start.size()) - 1;
            for (size_t l = 0; l < n_levels; l++) {
                const uint32_t a = P->z64 ? cc.level_start64[l] : cc.level_start[l], b = P->z64 ? cc.level_start64[l + 1] : cc.level_start[l + 1];
                for (uint32_t i = a; i < b; i++) {
                    uint64_t ep;
                    if (P->z64) {
                        if (cc.gates64[i].op != G64_MUL) continue;
                        ep = cc.gates64[i].ep;
                    } else {
                        if (g_op(cc.gates[i]) != G_MUL) continue;
                        ep = cc.gates[i].ep;
                    }
                    if (ep < row1 && l > ch.ready_level) good = false;  // (rows below the chunk count too: chunks leave in order)
                    if (ep >= row0 && ep < row1 && l == ch.ready_level) at_ready = true;
                }
            }
            // (a chunk whose own last writer is earlier than a previous chunk's inherits that chunk's level: in-order delivery)
            if (!at_ready && !(k && ch.ready_level == P->chunks[k - 1].ready_level)) good = false;
            if (k && ch.ready_level < P->chunks[k - 1].ready_level) good = false;
            if (k && ch.byte0 != P->chunks[k - 1].byte0 + P->chunks[k - 1].nbytes) good = false;
        }
        out[5] = good;
        return RV_OK;
    });
}

// Early corrections, device side.  early_flush (called by the level loop) puts, behind the level that completes a chunk, the
// packing kernel and a stamp kernel into the interpreter's own stream; the host -- idle once a proof is queued -- sees the
// stamp in the mapped mailbox and hands the chunk's copy to the second stream (early_pump), which therefore only ever
// holds copy-engine work and the "arrived" stamps.  Measured on the 10^7-gate circuit (tools/early_ab.py, gpurun_out/e*.log):
//  * packing kernels on the second stream are not dispatched while the first stream issues its short level launches back
//    to back (kernel trace: the first one starts when the hash kernels do), so the copies piled up behind the challenge;
//    in the interpreter's stream they cost 6 x 26 us;
//  * HIP events instead of stamps (hipEventRecord + hipStreamWaitEvent, or hipEventQuery from the host) were no cheaper, and
//    neither was a second stream of the highest priority;
//  * the packing kernel takes ~27 us per 27 MB chunk whatever its instruction count (a lane per repetition with multiplications,
//    or the 8 x 8 bit transposes it has now: 2 300 vs 700 instructions per thread): one generation of workgroups that all
//    load, then all store; its tiles as extra workgroups at the end of the level launches' grids (k_interp_full with a packing
//    branch, built and measured: byte-identical) cost the interpreter the same ~0.15 ms -- it has no idle issue slots to give;
//  * NOTHING may wait on the second stream.  Its copies were first followed by an "arrived" stamp kernel each (before that by an
//    event): a packet that waits for the copy engine's signal at the head of another hardware queue is polled by the command
//    processor between the first queue's level launches, and the 163 launches paid 0.2 ms for it (interpreter phase 2.40 - 2.45 ms
//    against 2.17 - 2.2 now; tools/copy_beside.py: copy-engine transfers alone beside the levels cost 0.03 ms).  The host waits for
//    the stream itself after the challenge -- a signal wait on the host side, no packet.
static int early_flush_chunks(rv_shard* s, size_t last) {
    EarlyRun* e = s->ec;
    rv_ctx* ctx = s->ctx;
    const auto& chunks = e->plan->chunks;
    if (e->next >= chunks.size() || last <= e->next) return RV_OK;
    // every chunk is packed in the interpreter's own stream (Z64: nothing to pack, the rows are the vectors)
    // (these launches sit inside the interpreter's phase but are not level launches: rv_profile counts them in slot 6)
    for (size_t k = e->next; k < last && !e->plan->z64; k++) {
        const auto& ch = chunks[k];
        launch_pack_corr_all(ctx->stream, s->d_pre, s->c->cc.n_pre, ch.byte0, ch.nbytes, ch.pitch, e->d_ec + ch.off);
        if (ctx->profiling) ctx->prof.launches[RV_PH_EARLY]++;
    }
    launch_publish(ctx->stream, nullptr, 0, nullptr, e->box_dev + 1, (e->seq << 8) | (uint32_t)last);
    if (ctx->profiling) ctx->prof.launches[RV_PH_EARLY]++;
    e->next = last;
    return RV_OK;
}
// level-synchronous schedule: the chunks whose preprocessing rows are final once `levels_queued` levels are in the stream
static int early_flush(rv_shard* s, size_t levels_queued) {
    EarlyRun* e = s->ec;
    const auto& chunks = e->plan->chunks;
    if (e->next >= chunks.size() || chunks[e->next].ready_level >= levels_queued) return RV_OK;
    size_t last = e->next;
    while (last < chunks.size() && chunks[last].ready_level < levels_queued) last++;
    return early_flush_chunks(s, last);
}

// The host's waits of the early-corrections path (a chunk's stamp, the challenge): the mailbox is written by the GPU, so there is
// nothing to block on -- but the caller need not burn a core for the milliseconds a proof takes either.  The wait SLEEPS through
// most of what the same wait took last time on this context (`ema_us`, a running average per kind of wait: proofs of one circuit
// repeat their timing to a few percent), then spins for the rest, so the word is seen as promptly as before.  Bounded: a stream that has ENDED (or failed) without the awaited word is RV_E_DEVICE at once; one still running is given
// ten times RV_EARLY_TIMEOUT_MS (default 20 000) -- a slow proof on a shared GPU is not a lost one -- then RV_E_DEVICE with a message, not a hang.
template <class Pred>
static int mailbox_wait(rv_ctx* ctx, Pred arrived, double* ema_us, const char* what) {
    static const long timeout_ms = getenv("RV_EARLY_TIMEOUT_MS") ? std::max(atol(getenv("RV_EARLY_TIMEOUT_MS")), 1l) : 20000;
    const auto t0 = std::chrono::steady_clock::now();
    auto elapsed_us = [&] { return std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count(); };
    if (ema_us && *ema_us > 200.0) {
        // sleep until ~80 % of the expected wait (minus the scheduler's slack) is over, in naps short enough to notice an early word
        const double until = 0.8 * *ema_us - 80.0;
        while (!arrived()) {
            const double left = until - elapsed_us();
            if (left < 30.0) break;
            timespec ts{0, (long)(std::min(left, 250.0) * 1000.0)};
            nanosleep(&ts, nullptr);
        }
    }
    int rc = RV_OK;
    for (uint64_t spins = 0; !arrived(); spins++) {
        __builtin_ia32_pause();
        if ((spins & 0xFFFF) == 0xFFFF) {
            const hipError_t q = hipStreamQuery(ctx->stream);
            if (q != hipErrorNotReady && !arrived()) {
                rc = q == hipSuccess ? RV_E_DEVICE : hip_fail(q, what, __FILE__, __LINE__);
                break;
            }
            // (a stream that is still RUNNING on a shared or oversubscribed GPU is slow, not lost: ten times the limit before giving up on it)
            if (elapsed_us() > 1e3 * (double)timeout_ms * 10.0) {
                g_last_error = std::string(what) + ": no word from a still running stream within 10 x RV_EARLY_TIMEOUT_MS (" + std::to_string(10ull * timeout_ms) + " ms)";
                rc = RV_E_DEVICE;
                break;
            }
        }
    }
    if (rc == RV_OK && ema_us) *ema_us = *ema_us > 0 ? 0.7 * *ema_us + 0.3 * elapsed_us() : elapsed_us();
    return rc;
}

// host side: waits for every chunk's stamp in turn and queues its copy to the host
static int early_pump(rv_shard* s) {
    EarlyRun* e = s->ec;
    rv_ctx* ctx = s->ctx;
    const auto& chunks = e->plan->chunks;
    for (; e->pumped < chunks.size(); e->pumped++) {
        const size_t k = e->pumped;
        if (k >= e->next) return RV_E_DEVICE;
        if (int rcw = mailbox_wait(ctx, [&] { return e->ready(k); }, k < 16 ? &ctx->ec_wait_us[k] : nullptr, "early corrections (pump)")) return rcw;
        const auto& ch = chunks[k];
        if (e->plan->z64) {
            // word range [byte0, byte0 + nbytes) of the first r_spec repetitions' preprocessing rows (16-byte multiples on both
            // sides: the copy engine's fast 2-D path)
            HIPCHK(hipMemcpy2DAsync(e->h_ec + ch.byte0, ch.pitch, (const uint8_t*)s->d_pre64 + ch.byte0, (size_t)s->c->cc.pre_words64 * 8, ch.nbytes,
                                    e->plan->r_spec, hipMemcpyDeviceToHost, ctx->stream2));
        } else {
            HIPCHK(hipMemcpyAsync(e->h_ec + ch.off, e->d_ec + ch.off, (size_t)e->plan->r_spec * ch.pitch, hipMemcpyDeviceToHost, ctx->stream2));
        }
        // (NO kernel or event behind the copy: a packet that waits for the copy engine's signal at the head of the second queue is
        // polled by the command processor between the first queue's level launches and costs the interpreter 0.15 - 0.2 ms per proof --
        // tools/copy_beside.py: copies alone beside the levels cost 0.03.  The host waits for the stream instead, after the challenge.)
    }
    return RV_OK;
}


static int shard_run_levels(rv_shard* s, int mode, const InterpParams& p, const Interp64Params& p64) {
    rv_ctx* ctx = s->ctx;
    const Compiled& cc = s->c->cc;
    const bool has64 = !cc.gates64.empty();
    hipStream_t sb = ctx->stream;
    const size_t n_levels = cc.level_start.empty() ? 0 : cc.level_start.size() - 1;
    ctx->phase(RV_PH_INTERP, sb);
    size_t waited = 0;  // mask chunks already waited for
    int rc_ec;
    const uint32_t n_qg64 = s->z64f ? s->NQ / z64_fused_qw(s->NQ) : 0;
    auto fused_params = [&](uint32_t qg0, uint32_t qgn) {
        Z64FParams zp{};
        zp.rk = s->d_keys64 ? s->d_rk64 : s->d_rk;
        zp.NQ = s->NQ;
        zp.wmask = p64.wmask;
        zp.masks = s->d_masks64;
        zp.on = p64.on;
        zp.pre = p64.pre;
        zp.on_words = p64.on_words;
        zp.pre_words = p64.pre_words;
        zp.wit = p64.wit;
        zp.v = s->d_v64;
        zp.err = p64.err;
        zp.first_block = 0;
        zp.qg0 = qg0;
        zp.qgn = qgn;
        if (mode == MODE_VERIFY) {
            zp.omit = p64.omit;
            zp.keep = s->d_keep64z;
            zp.wcorr = p64.wcorr;
            zp.sup_in = p64.sup_in;
            zp.sup_corr = p64.sup_corr;
            zp.sup_rec = p64.sup_rec;
            zp.sup_r = p64.sup_r;
        }
        return zp;
    };
    if (s->z64f && s->ev_sup64 && mode == MODE_VERIFY) {
        // (api: rv_verify_shard_impl, split64) the quad groups without an opened repetition first, every level; then, once the
        // supplied values are there, the first one
        for (int pass = 0; pass < 2; pass++) {
            if (pass == 1) {
                int rcm = s->mid64 ? s->mid64() : RV_OK;  // (the proof's copy and the unpack kernels, side stream)
                s->mid64 = nullptr;
                if (rcm) return rcm;
                HIPCHK(hipStreamWaitEvent(sb, s->ev_sup64, 0));
            }
            const Z64FParams zp = pass == 0 ? fused_params(1, n_qg64 - 1) : fused_params(0, 1);
            for (size_t l = 0; l < n_levels; l++)
                if (cc.level_start64[l + 1] > cc.level_start64[l]) {
                    launch_z64_fused(sb, s->c->d_gates64f, s->c->z64f_levels[l], zp);
                    ctx->count();
                }
        }
        return RV_OK;
    }
    auto ht_last = std::chrono::steady_clock::now();
    for (size_t l = 0; l < n_levels; l++) {
        if (g_ht.on) {
            const auto now = std::chrono::steady_clock::now();
            if (std::chrono::duration<double, std::milli>(now - ht_last).count() > 2) g_ht.mark("(slow: level iteration)");
            ht_last = now;
        }
        if (s->ec && (rc_ec = early_flush(s, l))) return rc_ec;
        if (s->overlap) {
            // (a run of levels in one launch needs its last level's masks)
            size_t l_need = l;
            if (s->c->lds_run_of_level[l] >= 0) l_need = std::max(l_need, (size_t)s->c->lds_runs[(size_t)s->c->lds_run_of_level[l]].run.l1 - 1);
            if (s->c->run_of_level[l] >= 0) l_need = std::max(l_need, (size_t)s->c->narrow_runs[(size_t)s->c->run_of_level[l]].second - 1);
            if ((rc_ec = overlap_need(s, cc.level_need_blocks[l_need], sb))) return rc_ec;
            waited = s->mask_chunks.size();
        }
        while (waited < s->mask_chunks.size() &&
               (waited == 0 ? 0 : s->mask_chunks[waited - 1].first) < cc.level_need_blocks[l]) {
            HIPCHK(hipStreamWaitEvent(sb, s->mask_chunks[waited].second, 0));
            waited++;
        }
        const bool own_launch = mode == MODE_PROVE_V || mode == MODE_VERIFY_C;  // (these modes exist in the one-launch-per-level kernel only)
        if (!own_launch && s->c->lds_run_of_level[l] >= 0 && lds_run_fits_rows(s->c->lds_runs[(size_t)s->c->lds_run_of_level[l]].qs, p.NQ)) {
            // a narrow stretch with its live wires in LDS: one launch, NQ / qs workgroups
            const auto& pl = s->c->lds_runs[(size_t)s->c->lds_run_of_level[l]];
            if (l == pl.run.l0) {
                while (waited < s->mask_chunks.size() &&
                       (waited == 0 ? 0 : s->mask_chunks[waited - 1].first) < cc.level_need_blocks[pl.run.l1 - 1]) {
                    HIPCHK(hipStreamWaitEvent(sb, s->mask_chunks[waited].second, 0));
                    waited++;
                }
                launch_interp_lds(sb, mode, pl.qs, p.NQ, s->c->d_lds_recs + pl.run.rec0, pl.run.n_steps, pl.run.n_slots, pl.run.eo0, pl.run.ep0, p, nullptr, 1);
                ctx->count();
            }
            continue;
        }
        if (s->c->run_of_level[l] >= 0 && !own_launch) {
            // a run of narrow levels: one launch for the whole run (its mask needs were waited for above
            // level by level as the loop advances, so wait for the run's last level first)
            const auto& run = s->c->narrow_runs[(size_t)s->c->run_of_level[l]];
            if (l == run.first) {
                while (waited < s->mask_chunks.size() &&
                       (waited == 0 ? 0 : s->mask_chunks[waited - 1].first) < cc.level_need_blocks[run.second - 1]) {
                    HIPCHK(hipStreamWaitEvent(sb, s->mask_chunks[waited].second, 0));
                    waited++;
                }
                launch_interp_narrow(sb, mode, s->c->d_gates, s->c->d_level_range, run.first, run.second, run.tiny, p);
                ctx->count();
            }
            continue;
        }
        if (cc.level_start[l + 1] > cc.level_start[l]) {
            // the level that follows as a launch of its own (not a narrow run) gets its first gate records prefetched
            const LevelRange* next = (l + 1 < n_levels && (s->c->run_of_level[l + 1] < 0 || own_launch) && cc.level_start[l + 2] > cc.level_start[l + 1])
                                         ? &cc.level_range[l + 1]
                                         : nullptr;
            launch_interp(sb, mode, s->c->d_gates, cc.level_range[l], p, next);
            ctx->count();
        }
        if (has64 && cc.level_start64[l + 1] > cc.level_start64[l]) {
            if (s->z64f) {
                const Z64FParams zp = fused_params(0, n_qg64);
                    launch_z64_fused(sb, s->c->d_gates64f, s->c->z64f_levels[l], zp);
            } else {
                launch_interp64(sb, mode, s->c->d_gates64, cc.level_start64[l], cc.level_start64[l + 1], p64);
            }
            ctx->count();
        }
    }
    if (s->ec && (rc_ec = early_flush(s, n_levels))) return rc_ec;
    if (s->overlap && (rc_ec = overlap_need(s, s->ov_blocks, sb))) return rc_ec;  // (masks no level reads: padding)
    if (s->overlap && mode != MODE_VERIFY && mode != MODE_VERIFY_C) g_overlap_commits.fetch_add(1, std::memory_order_relaxed);  // (the verifier has its own schedule: RV_VERIFY_HEAD)
    if (g_ov_trace) g_ov_trace->mark("main: last level done", n_levels, sb);
    return RV_OK;
}

static int shard_run_hash(rv_shard* s) {
    rv_ctx* ctx = s->ctx;
    const Compiled& cc = s->c->cc;
    ctx->phase(RV_PH_HASH);
    uint32_t* dig = s->d_dig;
    const size_t DW = (size_t)s->R * 8;
    uint32_t n_launch;
    if (launch_b3_pair_small(ctx->stream, s->d_pre, cc.n_pre, s->d_on, cc.n_on, s->NQ, s->d_cv[0], s->d_cv[1], dig + 0 * DW, dig + 1 * DW,
                             s->d_on_quads, s->n_on_quads)) {
        n_launch = 2;  // short transcripts (small circuits): both streams in the same two launches
    } else if (s->d_cv2[0]) {
        n_launch = launch_b3_pair_big(ctx->stream, s->d_pre, cc.n_pre, s->d_on, cc.n_on, s->NQ, s->d_cv[0], s->d_cv[1], s->d_cv2[0], s->d_cv2[1], dig + 0 * DW, dig + 1 * DW,
                                      s->d_on_quads, s->n_on_quads);
    } else {
        n_launch = launch_b3_stream_bits(ctx->stream, s->d_pre, cc.n_pre, s->NQ, s->d_cv[0], s->d_cv[1], dig + 0 * DW);
        n_launch += launch_b3_stream(ctx->stream, s->d_on, cc.n_on, s->NQ, s->d_cv[0], s->d_cv[1], dig + 1 * DW, s->d_on_quads, s->n_on_quads);
    }
    // Z64 transcripts; for a pure GF(2) circuit both are empty and every digest is BLAKE3("") (one fill, not four launches)
    if (cc.pre_words64 == 0 && cc.on_words64 == 0) {
        if (!s->dig64_filled) {
            launch_fill_digests(ctx->stream, dig + 2 * DW, 2 * s->R, b3_empty_digest());
            n_launch += 1;
        }
    } else {
        n_launch += launch_b3_contig(ctx->stream, s->d_pre64, cc.pre_words64, s->R, s->d_cv[0], s->d_cv[1], dig + 2 * DW);
        n_launch += launch_b3_contig(ctx->stream, s->d_on64, cc.on_words64, s->R, s->d_cv[0], s->d_cv[1], dig + 3 * DW);
    }
    ctx->count(n_launch);
    ctx->phase(-1);
    return RV_OK;
}

static int shard_run(rv_shard* s, int mode, InterpParams& p, Interp64Params& p64) {
    int rc;
    if ((rc = shard_run_alloc(s, p, p64))) return rc;
    g_ht.mark("alloc");
    if ((rc = shard_run_levels(s, mode, p, p64))) return rc;
    g_ht.mark("levels");
    if ((rc = shard_run_hash(s))) return rc;
    g_ht.mark("hash");
    return RV_OK;
}

static int shard_join(rv_shard* s) {
    const size_t DW = (size_t)s->R * 8;
    s->ctx->phase(RV_PH_JOIN);
    s->ctx->count();
    launch_join(s->ctx->stream, s->d_dig, s->d_dig + DW, s->d_dig + 2 * DW, s->d_dig + 3 * DW, s->R, s->d_h);
    s->ctx->phase(-1);
    HIPCHK(hipGetLastError());
    return RV_OK;
}


extern "C" int rv_shard_digests_device(rv_shard* s, void** dptr) {
    if (!s || !dptr) return RV_E_ARG;
    *dptr = s->d_h;
    return RV_OK;
}

extern "C" int rv_shard_digests(rv_shard* s, uint8_t* out) {
    if (!s || !out) return RV_E_ARG;
    HIPCHK(hipMemcpyAsync(out, s->d_h, (size_t)s->R * 32, hipMemcpyDeviceToHost, s->ctx->stream));
    HIPCHK(hipStreamSynchronize(s->ctx->stream));
    return RV_OK;
}

extern "C" int rv_shard_digests_to_device(rv_shard* s, void* dst_device) {
    if (!s || !dst_device) return RV_E_ARG;
    HIPCHK(hipMemcpyAsync(dst_device, s->d_h, (size_t)s->R * 32, hipMemcpyDeviceToDevice, s->ctx->stream));
    HIPCHK(hipStreamSynchronize(s->ctx->stream));
    return RV_OK;
}

extern "C" int rv_hook_shard_stream_digests(rv_shard* s, uint8_t* out) {
    if (!s || !out) return RV_E_ARG;
    std::vector<uint32_t> tmp((size_t)4 * s->R * 8);
    HIPCHK(hipMemcpyAsync(tmp.data(), s->d_dig, tmp.size() * 4, hipMemcpyDeviceToHost, s->ctx->stream));
    HIPCHK(hipStreamSynchronize(s->ctx->stream));
    for (uint32_t r = 0; r < s->R; r++)
        for (int k = 0; k < 4; k++) memcpy(out + ((size_t)r * 4 + k) * 32, &tmp[((size_t)k * s->R + r) * 8], 32);
    return RV_OK;
}
