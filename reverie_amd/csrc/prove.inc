// Part of api.hip (#included there, one translation unit): rv_prove / rv_prove_device: Proof::new (proof/mod.rs:119-222) with the early-corrections path.

// dst (nullable): page-locked destination of at least dst_cap bytes supplied by the caller (rv_prove_batch hands every
// proof a slice of one buffer); otherwise the proof gets a buffer of its own
// allow_early: the early-corrections path may be taken (a one-shot rv_prove_ops does without: its staging buffer is 3x the proof
// of page-locked memory, tens of milliseconds to map for a gain of half a millisecond)
static int rv_prove_impl(rv_ctx* ctx, const rv_circuit* c, const WitSrc& w, const uint8_t* seeds, uint8_t** proof, size_t* proof_len,
                        uint8_t* dst = nullptr, size_t dst_cap = 0, bool allow_early = true);

extern "C" int rv_prove(rv_ctx* ctx, const rv_circuit* c, const uint8_t* wit_gf2, size_t n_gf2, const uint64_t* wit_z64,
                        size_t n_z64, const uint8_t* seeds, uint8_t** proof, size_t* proof_len) {
    try {  // no C++ exception may cross the C boundary
        return rv_prove_impl(ctx, c, wit_host(wit_gf2, n_gf2, wit_z64, n_z64), seeds, proof, proof_len);
    } catch (...) {
        g_last_error = "out of host memory";
        return RV_E_NOMEM;
    }
}

// (RV_BATCH_STATS: when the calling thread's last plain-path proof had its commitment queued, its openings queued, its stream done -- ms since entry)
static thread_local double g_prove_marks[3];
static int rv_prove_impl(rv_ctx* ctx, const rv_circuit* c, const WitSrc& w, const uint8_t* seeds, uint8_t** proof, size_t* proof_len, uint8_t* dst,
                        size_t dst_cap, bool allow_early) {
    LibBusy busy_guard;  // (compile.h: the background unmapper keeps still while the GPU is driven)
    if (!ctx || !c || !proof || !proof_len) return RV_E_ARG;
    *proof = nullptr;
    *proof_len = 0;
    uint8_t os_seeds[RV_TOTAL_REPS * RV_KEY_SIZE];
    if (!seeds) {  // proof/mod.rs:131-134 uses OsRng
        size_t got = 0;
        while (got < sizeof os_seeds) {
            ssize_t n = getrandom(os_seeds + got, sizeof os_seeds - got, 0);
            if (n <= 0) return RV_E_DEVICE;
            got += (size_t)n;
        }
        seeds = os_seeds;
    }
    rv_shard* s = nullptr;
    uint8_t* out = nullptr;
    // Early corrections (open.hip): half of a large GF(2) proof -- the corrections vectors -- does not depend on the
    // challenge beyond the choice of repetitions.  Every repetition's vector goes to a page-locked staging buffer through
    // the copy engine while the interpreter and the hash kernels run; once the challenge is known (published into a mapped
    // mailbox the host polls, no stream synchronisation) helper threads copy the 40 opened ones into the proof while the GPU
    // extracts the other half, which a kernel then writes around them into the same buffer.  RV_EARLY=0 turns it off.
    EarlyRun er;
    bool early = false;
    double g_prove_t0 = 0;  // when the commit phase began, from the call's start (ms)
    const bool early_stats = getenv("RV_EARLY_STATS") && atoi(getenv("RV_EARLY_STATS"));
    const auto t_begin = std::chrono::steady_clock::now();
    auto since = [&] { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_begin).count(); };
    double t_queued = 0, t_chal = 0, t_copied = 0, t_sync = 0;
    std::vector<double> t_chunk;
    uint8_t* out_dev = nullptr;
    uint32_t* fs_dev = nullptr;
    OpenLayout EL{};
    const bool early_on = !(getenv("RV_EARLY") && atoi(getenv("RV_EARLY")) == 0);
    if (early_on && allow_early && !dst && !g_recorder) {
        const EarlyPlan* pl = early_plan(c);
        if (pl->ok) {
            HIPCHK(hipSetDevice(ctx->device));
            uint8_t canon[RV_TOTAL_REPS];
            for (uint32_t r = 0; r < RV_TOTAL_REPS; r++) canon[r] = r < RV_ONLINE_REPS ? 0 : RV_PLAYERS;
            EL = open_layout(c->cc, canon, RV_TOTAL_REPS, true);
            bool ok = ctx_stream2(ctx) == RV_OK;
            if (ctx->h_ec_cap < pl->bytes) {
                if (ctx->h_ec) (void)hipHostFree(ctx->h_ec);
                ctx->h_ec = nullptr;
                ctx->h_ec_cap = 0;
                if (hipHostMalloc((void**)&ctx->h_ec, pl->bytes, hipHostMallocDefault) == hipSuccess)
                    ctx->h_ec_cap = pl->bytes;
                else
                    ok = false;
            }
            if (ok && !pl->z64 && ctx->d_ec_cap < pl->bytes) {
                if (ctx->d_ec) (void)hipFree(ctx->d_ec);
                ctx->d_ec = nullptr;
                ctx->d_ec_cap = 0;
                if (hipMalloc((void**)&ctx->d_ec, pl->bytes) == hipSuccess)
                    ctx->d_ec_cap = pl->bytes;
                else
                    ok = false;
            }
            if (ok && !ctx->h_fs) {
                if (hipHostMalloc((void**)&ctx->h_fs, 4096, hipHostMallocMapped) == hipSuccess)
                    memset(ctx->h_fs, 0, 4096);
                else
                    ok = false;
            }
            if (ok && hipHostGetDevicePointer((void**)&fs_dev, ctx->h_fs, 0) != hipSuccess) ok = false;
            if (!ok) (void)hipGetLastError();
            if (ok && !ctx->ec_pool) {
                constexpr int n_helpers = 9;
                ctx->ec_pool = new HelperPool(n_helpers);
            }
            // (test knob: the staging buffer starts every proof as garbage, so that bytes copied out of it before they arrived show)
            if (ok && getenv("RV_EARLY_POISON") && atoi(getenv("RV_EARLY_POISON"))) memset(ctx->h_ec, 0x5A, pl->bytes);
            if (ok) {
                early = true;
                er.plan = pl;
                er.h_ec = ctx->h_ec;
                er.d_ec = ctx->d_ec;
                er.box_dev = fs_dev;
                er.box = ctx->h_fs;
                ctx->fs_seq = (ctx->fs_seq + 1) & 0xFFFFFFu;  // a fresh number even after a proof that failed half-way: its stamps must never match
                if (!ctx->fs_seq) ctx->fs_seq = 1;
                er.seq = ctx->fs_seq;
            }
        }
    }
    g_prove_t0 = since();
    g_ht.begin();
    int rc = rv_shard_commit_impl(ctx, c, w, seeds, 0, RV_TOTAL_REPS, &s, /*defer_sync=*/true, early ? &er : nullptr);
    g_ht.mark("commit");
    if (rc) return rc;
    g_prove_marks[0] = since();
    if (early) {
        // the proof's buffer, now that the GPU is busy (a fresh page-locked buffer of a 640 MB proof takes 45 ms to map).  Without it
        // the plain path below still works: the stamps in the stream are harmless, nothing was handed to the second stream yet
        if (!(out = (uint8_t*)out_alloc(EL.total)) || hipHostGetDevicePointer((void**)&out_dev, out, 0) != hipSuccess || ((uintptr_t)out_dev & 15)) {
            (void)hipGetLastError();
            rv_free(out);
            out = nullptr;
            early = false;
            s->ec = nullptr;
        }
    }
    if (early) do {
        void* d = nullptr;
        size_t lens[4];
        const uint32_t seq = er.seq;
        const bool z64 = er.plan->z64;
        // The broadcast vectors go to the proof buffer from the extraction kernel itself (internal.h: OpenDirect; DESIGN.md section 9.1),
        // k_copy_gaps behind it brings the rest of the image.  By default where the vectors are long enough for tiles of 64 bytes and
        // more; RV_OPEN_DIRECT=num/den (read at every call: the tests switch it): only that leading share of the tiles (0/1: none),
        // and whatever the tile (16 bytes at least)
        OpenDirect od;
        if (!z64) {
            unsigned n = 1, d = 1;
            const char* e = getenv("RV_OPEN_DIRECT");
            if (e && (sscanf(e, "%u/%u", &n, &d) != 2 || !d || n > d)) n = 0, d = 1;
            od.tile = extract_tile_bytes(c->cc.n_rec);
            od.rvec_at = 137;  // (k_fs_challenge: a record's broadcast vector follows its 129-byte head and an 8-byte length)
            od.rvec_len = EL.l2r;
            od.n_direct = (uint32_t)(((EL.l2r + od.tile - 1) / od.tile) * n / d);
            if (!od.n_direct || od.tile < (e ? 16u : 64u) || (od.tile & (od.tile - 1)))
                od = OpenDirect();
            else
                s->od_out = out_dev, s->od_n_direct = od.n_direct;
        }
        if ((rc = shard_open_impl(s, nullptr, nullptr, &d, lens, true, nullptr, nullptr, /*no_sync=*/true, nullptr, fs_dev, seq, z64 ? 0 : er.plan->r_spec,
                                  z64 ? er.plan->r_spec : 0)))
            break;
        const size_t total = 32 + 4 * 8 + lens[0] + lens[1] + lens[2] + lens[3];
        if (total != EL.total || er.packed.size() != er.plan->chunks.size() || er.plan->chunks.size() > 255) {
            rc = RV_E_DEVICE;
            break;
        }
        // the image without the corrections vectors, then the error word (mailbox word 8)
        // (Z64: only the records of the opened repetitions below r_spec -- the kernel counts them -- go without their vectors)
        const uint64_t corr_at = 145 + (z64 ? EL.l64r : EL.l2r);
        const uint64_t rec_first = z64 ? EL.base[2] : EL.base[0], rec_size = z64 ? EL.sz64 : EL.sz2, corr_len = z64 ? EL.l64c : EL.l2c;
        // (... and the error word, mailbox word 8, in the same launch)
        launch_copy_gaps(ctx->stream, (const uint8_t*)d, out_dev, total, rec_first, rec_size, corr_at, corr_len, RV_ONLINE_REPS, s->d_omit, er.plan->r_spec, od,
                         s->d_err, (int*)(fs_dev + 8));
        if (hipGetLastError() != hipSuccess) {
            rc = RV_E_DEVICE;
            break;
        }
        t_queued = since();
        if ((rc = early_pump(s))) break;
        // the challenge: poll the mailbox (now and then make sure the stream is still alive)
        volatile uint32_t* box = ctx->h_fs;
        if ((rc = mailbox_wait(ctx, [&] { return __atomic_load_n(&box[0], __ATOMIC_ACQUIRE) == seq; }, &ctx->ec_wait_us[16], "early corrections (challenge)"))) break;
        t_chal = since();
        const uint8_t* omit_all = (const uint8_t*)(ctx->h_fs + 16) + 32;
        uint32_t opened[RV_ONLINE_REPS], n_open = 0;
        for (uint32_t r = 0; r < RV_TOTAL_REPS; r++)
            if (omit_all[r] < RV_PLAYERS && n_open < RV_ONLINE_REPS) opened[n_open++] = r;
        // the copies of the chunks: normally long done; the host waits for the second stream (its copies complete in order), then every
        // thread (this one included) claims (chunk, opened repetition) pieces from one counter: a helper that wakes up late takes fewer
        // pieces instead of holding its share back
        if (hipStreamSynchronize(ctx->stream2) != hipSuccess) {
            rc = hip_fail(hipGetLastError(), "early corrections (copies)", __FILE__, __LINE__);
            break;
        }
        if (early_stats) t_chunk.push_back(since());
        {
            const auto& chunks = er.plan->chunks;
            std::atomic<size_t> next_piece{0};
            std::atomic<int> bad{0};
            // (Z64: the staging buffer holds the first r_spec repetitions; the opened ones among them are the first n_staged ranks)
            uint32_t n_staged = 0;
            for (uint32_t j = 0; j < n_open; j++)
                if (opened[j] < er.plan->r_spec) n_staged = j + 1;
            const size_t n_pieces = chunks.size() * n_staged;
            const std::function<void(int)> job = [&](int t) {
                for (;;) {
                    const size_t t = next_piece.fetch_add(1, std::memory_order_relaxed);
                    if (t >= n_pieces) return;
                    const size_t k = t / n_staged, j = t % n_staged;
                    const auto& ch = chunks[k];
                    memcpy(out + rec_first + j * rec_size + corr_at + ch.byte0, er.h_ec + ch.off + (size_t)opened[j] * ch.pitch + (z64 ? ch.byte0 : 0), ch.nbytes);
                }
            };
            ctx->ec_pool->run(job);
            t_copied = since();
            if (bad.load()) {
                rc = hip_fail(hipGetLastError(), "early corrections (copy)", __FILE__, __LINE__);
                break;
            }
        }
        if (hipStreamSynchronize(ctx->stream) != hipSuccess) {
            rc = hip_fail(hipGetLastError(), "proof (early corrections)", __FILE__, __LINE__);
            break;
        }
        t_sync = since();
        if (early_stats) {
            fprintf(stderr, "early: queued %.3f  challenge %.3f  chunks", t_queued, t_chal);
            for (double t : t_chunk) fprintf(stderr, " %.3f", t);
            fprintf(stderr, "  copied %.3f  stream done %.3f ms", t_copied, t_sync);
            for (auto& m : g_ht.marks) fprintf(stderr, "  [%s %.3f]", m.first, m.second + g_prove_t0);  // (RV_BATCH_STATS=1: the host's own marks)
            fprintf(stderr, "\n");
        }
        ctx->collect();
        if (n_open != RV_ONLINE_REPS) {
            rc = RV_E_DEVICE;
            break;
        }
        if ((int)ctx->h_fs[8]) {
            rc = RV_E_WITNESS_INVALID;
            break;
        }
        size_t off = 32;
        const uint64_t counts[4] = {RV_ONLINE_REPS, RV_PREPROCESSING_REPS, RV_ONLINE_REPS, RV_PREPROCESSING_REPS};
        for (int k = 0; k < 4; k++) {
            put_le64(out + off, counts[k]);
            off += 8 + lens[k];
        }
        *proof = out;
        *proof_len = total;
        out = nullptr;
        g_early_proofs.fetch_add(1, std::memory_order_relaxed);
        if (od.n_direct) g_open_direct_proofs.fetch_add(1, std::memory_order_relaxed);
    } while (0);
    else do {
        // commitment, challenge and openings all on the device (k_fs_challenge); the whole proof is laid out there
        // in its final bincode form (comm included) and leaves in ONE copy; the host waits for the device once
        void* d = nullptr;
        size_t lens[4];
        // small proofs: straight into the context's mapped staging buffer (the layout of a whole proof does not depend on
        // the challenge, so its size is known before the openings exist)
        constexpr bool small_stage = true;
        uint8_t* stage_dev = nullptr;
        size_t need = 0;
        if (small_stage && !g_recorder) {
            uint8_t canon[RV_TOTAL_REPS];
            for (uint32_t r = 0; r < RV_TOTAL_REPS; r++) canon[r] = r < RV_ONLINE_REPS ? 0 : RV_PLAYERS;
            need = open_layout(c->cc, canon, RV_TOTAL_REPS, true).total;
            if (need + 64 <= rv_ctx::STAGE_BYTES) {
                if (!ctx->h_stage && hipHostMalloc((void**)&ctx->h_stage, rv_ctx::STAGE_BYTES, hipHostMallocMapped) != hipSuccess) {
                    (void)hipGetLastError();
                    ctx->h_stage = nullptr;
                }
                if (ctx->h_stage && hipHostGetDevicePointer((void**)&stage_dev, ctx->h_stage, 0) != hipSuccess) {
                    (void)hipGetLastError();
                    stage_dev = nullptr;
                }
            }
        }
        if (stage_dev) s->err_dst_mapped = (int*)(stage_dev + ((need + 15) & ~(size_t)15));  // (the openings' launch may carry the error word)
        if ((rc = shard_open_impl(s, nullptr, stage_dev, &d, lens, true, nullptr, nullptr, /*no_sync=*/true))) break;
        const size_t total = 32 + 4 * 8 + lens[0] + lens[1] + lens[2] + lens[3];
        if (dst && total > dst_cap) {
            rc = RV_E_ARG;
            break;
        }
        out = dst ? dst : (uint8_t*)out_alloc(total);
        if (!out) {
            rc = RV_E_NOMEM;
            break;
        }
        int err = 0;
        g_ht.mark("open");
        g_prove_marks[1] = since();
        if (stage_dev) {
            if (total != need) {
                rc = RV_E_DEVICE;
                break;
            }
            const size_t err_at = (total + 15) & ~(size_t)15;
            if (!s->err_word_sent) launch_store_word(ctx->stream, s->d_err, (int*)(stage_dev + err_at));
            if (hipStreamSynchronize(ctx->stream) != hipSuccess) {
                rc = hip_fail(hipGetLastError(), "proof (staged)", __FILE__, __LINE__);
                break;
            }
            memcpy(&err, ctx->h_stage + err_at, sizeof err);
            memcpy(out, ctx->h_stage, total);
        } else if (hipMemcpyAsync(out, d, total, hipMemcpyDeviceToHost, ctx->stream) != hipSuccess ||
                   hipMemcpyAsync(&err, s->d_err, sizeof err, hipMemcpyDeviceToHost, ctx->stream) != hipSuccess ||
                   hipStreamSynchronize(ctx->stream) != hipSuccess) {
            rc = hip_fail(hipGetLastError(), "proof D2H", __FILE__, __LINE__);
            break;
        }
        g_prove_marks[2] = since();
        ctx->collect();
        if (err) {
            rc = RV_E_WITNESS_INVALID;
            break;
        }
        size_t off = 32;
        const uint64_t counts[4] = {RV_ONLINE_REPS, RV_PREPROCESSING_REPS, RV_ONLINE_REPS, RV_PREPROCESSING_REPS};
        for (int k = 0; k < 4; k++) {
            put_le64(out + off, counts[k]);
            off += 8 + lens[k];
        }
        *proof = out;
        *proof_len = total;
        out = nullptr;
    } while (0);
    const double t_before_destroy = since();
    rv_shard_destroy(s);  // (waits for both streams: nothing writes into `out` any more)
    if (!dst) rv_free(out);
    if (early_stats) fprintf(stderr, "early: shard released %.3f -> %.3f ms\n", t_before_destroy, since());
    return rc;
}

static int rv_prove_device_impl(rv_ctx* ctx, const rv_circuit* c, const WitSrc& w, const uint8_t* seeds, void* dst_device, uint8_t comm[RV_HASH_SIZE],
                                uint8_t omit[RV_TOTAL_REPS], size_t lens[4]) {
    LibBusy busy_guard;  // (compile.h: the background unmapper keeps still while the GPU is driven)
    if (!ctx || !c || !seeds || !dst_device || !comm || !omit || !lens) return RV_E_ARG;
    rv_shard* s = nullptr;
    int rc = rv_shard_commit_impl(ctx, c, w, seeds, 0, RV_TOTAL_REPS, &s, /*defer_sync=*/true);
    if (rc) return rc;
    do {
        void* d = nullptr;
        if ((rc = shard_open_impl(s, nullptr, dst_device, &d, lens, false, nullptr, nullptr, /*no_sync=*/true))) break;
        uint8_t back[RV_TOTAL_REPS + 32];  // omit of the (whole) shard, then comm
        int err = 0;
        if (hipMemcpyAsync(back, s->d_omit, sizeof back, hipMemcpyDeviceToHost, ctx->stream) != hipSuccess ||
            hipMemcpyAsync(&err, s->d_err, sizeof err, hipMemcpyDeviceToHost, ctx->stream) != hipSuccess ||
            hipStreamSynchronize(ctx->stream) != hipSuccess) {
            rc = hip_fail(hipGetLastError(), "rv_prove_device", __FILE__, __LINE__);
            break;
        }
        ctx->collect();
        if (err) {
            rc = RV_E_WITNESS_INVALID;
            break;
        }
        memcpy(omit, back, RV_TOTAL_REPS);
        memcpy(comm, back + RV_TOTAL_REPS, 32);
    } while (0);
    rv_shard_destroy(s);
    return rc;
}

extern "C" int rv_prove_device(rv_ctx* ctx, const rv_circuit* c, const uint8_t* wit_gf2, size_t n_gf2, const uint64_t* wit_z64,
                               size_t n_z64, const uint8_t* seeds, void* dst_device, uint8_t comm[RV_HASH_SIZE],
                               uint8_t omit[RV_TOTAL_REPS], size_t lens[4]) {
    try {  // no C++ exception may cross the C boundary
        return rv_prove_device_impl(ctx, c, wit_host(wit_gf2, n_gf2, wit_z64, n_z64), seeds, dst_device, comm, omit, lens);
    } catch (...) {
        g_last_error = "out of host memory";
        return RV_E_NOMEM;
    }
}
