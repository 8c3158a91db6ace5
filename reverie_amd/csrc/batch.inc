// Part of api.hip (#included there, one translation unit): rv_prove_batch.

// ------------------------------------------------------------------------------------
// rv_prove_batch: `batch` proofs of ONE circuit, different witnesses and seeds, in one pass.
// Deep narrow circuits (AES, SHA: thousands of dependency levels of a few gates) are latency-bound: one proof keeps
// a single workgroup busy, and proofs in flight on separate contexts stop scaling at ~16 (host launch overhead).
// Here every level / narrow-run launch carries all proofs (grid.y resp. one workgroup per proof), so the latency
// chain is paid once per batch; the per-proof phases around it (keys, masks, digests, openings) are queued proof
// after proof on the same stream with a single synchronisation at the end.
// ------------------------------------------------------------------------------------
// Issues the calls recorded for the proofs of a batch (launch.h): every kernel step once, with gridDim.y = proof and
// the argument blocks in a device array; recorded copies one by one.  The staging buffers go to the caller's lists.
static int replay_recorded(rv_ctx* ctx, std::vector<LaunchRecorder>& recs, std::vector<void*>& pinned_tmp, std::vector<void*>& device_tmp) {
    const size_t batch = recs.size(), n = recs[0].calls.size();
    for (size_t b = 1; b < batch; b++)
        if (recs[b].calls.size() != n) return RV_E_DEVICE;
    size_t total = 0;
    std::vector<size_t> off(n, 0);
    for (size_t i = 0; i < n; i++) {
        const auto& c0 = recs[0].calls[i];
        for (size_t b = 1; b < batch; b++) {
            const auto& c = recs[b].calls[i];
            if (c.replay != c0.replay || c.fill != c0.fill || c.grid.x != c0.grid.x || c.block.x != c0.block.x || c.arg_bytes != c0.arg_bytes) return RV_E_DEVICE;
        }
        if (!c0.replay) continue;
        if (c0.grid.y != 1 || c0.grid.z != 1) return RV_E_DEVICE;
        off[i] = total;
        total += ((size_t)c0.arg_bytes * batch + 15) & ~(size_t)15;
    }
    uint8_t* d_args = nullptr;
    if (total) {
        uint8_t* h = (uint8_t*)g_pinned.get(std::max<size_t>(total, PinnedPool::MIN_BYTES));
        if (!h) return RV_E_NOMEM;
        pinned_tmp.push_back(h);
        for (size_t i = 0; i < n; i++) {
            const uint32_t ab = recs[0].calls[i].arg_bytes;
            if (!recs[0].calls[i].replay) continue;
            for (size_t b = 0; b < batch; b++) memcpy(h + off[i] + b * ab, recs[b].calls[i].args.data(), ab);
        }
        int r = dalloc(ctx, total, &d_args);
        if (r) return r;
        device_tmp.push_back(d_args);
        if (hipMemcpyAsync(d_args, h, total, hipMemcpyHostToDevice, ctx->stream) != hipSuccess) return RV_E_DEVICE;
    }
    for (size_t i = 0; i < n; i++) {
        const auto& c0 = recs[0].calls[i];
        if (c0.replay) {
            c0.replay(ctx->stream, c0.grid, c0.block, d_args + off[i], (unsigned)batch);
        } else {
            for (size_t b = 0; b < batch; b++) {
                const auto& c = recs[b].calls[i];
                if ((c.fill ? hipMemsetAsync(c.dst, c.value, c.n, ctx->stream) : hipMemcpyAsync(c.dst, c.src, c.n, c.kind, ctx->stream)) != hipSuccess)
                    return RV_E_DEVICE;
            }
        }
    }
    if (hipGetLastError() != hipSuccess) return RV_E_DEVICE;
    for (auto& r : recs) r.calls.clear();
    return RV_OK;
}

// Circuits from this many gates on (GF(2) and Z64 gates counted together where the circuit has Z64 gates) leave the one-pass
// path of rv_prove_batch and rv_verify_batch (RV_BATCH_BIG_GATES, default 2^20)
static size_t batch_big_gates() {
    static const size_t n = [] {
        const char* e = getenv("RV_BATCH_BIG_GATES");
        return e ? (size_t)strtoull(e, nullptr, 10) : (size_t)1 << 20;
    }();
    return n;
}

// All proofs of a one-pass batch level by level (mode: MODE_PROVE / MODE_VERIFY; d_pp64 only for Z64 / mixed circuits), in the
// order of shard_run_levels: per level the GF(2) launch, then the Z64 one.  LDS and narrow runs cover levels without Z64 gates
// only -- rv_circuit's run plans -- so the levels they `continue` past have no Z64 launch to skip.  Z64 / mixed circuits count
// one launch per batched launch, whatever the batch size.
static void launch_levels_batched(rv_ctx* ctx, const rv_circuit* c, int mode, const InterpParams* d_pp, const Interp64Params* d_pp64, size_t batch) {
    const Compiled& cc = c->cc;
    const bool has64 = !cc.gates64.empty();
    const size_t n_levels = cc.level_start.empty() ? 0 : cc.level_start.size() - 1;
    for (size_t l = 0; l < n_levels; l++) {
        if (lds_run_for_batch(c, l, batch)) {
            const auto& pl = c->lds_runs[(size_t)c->lds_run_of_level[l]];
            if (l == pl.run.l0) {
                launch_interp_lds(ctx->stream, mode, pl.qs, RV_TOTAL_REPS / 4, c->d_lds_recs + pl.run.rec0, pl.run.n_steps, pl.run.n_slots,
                                  pl.run.eo0, pl.run.ep0, InterpParams{}, d_pp, (uint32_t)batch);
                if (has64) ctx->count();
            }
            continue;
        }
        if (c->run_of_level[l] >= 0) {
            const auto& run = c->narrow_runs[(size_t)c->run_of_level[l]];
            if (l == run.first) {
                launch_interp_narrow_batched(ctx->stream, c->d_gates, c->d_level_range, run.first, run.second, run.tiny, d_pp, (uint32_t)batch, mode);
                if (has64) ctx->count();
            }
            continue;
        }
        launch_interp_batched(ctx->stream, c->d_gates, cc.level_range[l], d_pp, (uint32_t)batch, mode);
        if (has64 && cc.level_start[l + 1] > cc.level_start[l]) ctx->count();
        if (has64 && cc.level_start64[l + 1] > cc.level_start64[l]) {
            launch_interp64_batched(ctx->stream, mode, c->d_gates64, cc.level_start64[l], cc.level_start64[l + 1], d_pp64, (uint32_t)batch);
            ctx->count();
        }
    }
}

// Where a batch's proofs go.  rv_prove_batch: page-locked host buffers, proofs[b] / proof_lens[b].  rv_prove_batch_device
// (d_dst set, proofs and proof_lens null): the caller's device buffer, proof b framed at d_dst + b * stride -- its entry point
// has checked the buffer against the proof length -- and no proof byte goes to the host.
struct BatchDst {
    uint8_t** proofs;
    size_t* proof_lens;
    uint8_t* d_dst;
    size_t stride;
};

// One proof, framed, straight into device memory at d_dst (rv_prove_batch_device's proof-after-proof branch): the error word is
// all the host waits for.
static int prove_framed_device(rv_ctx* ctx, const rv_circuit* c, const WitSrc& w, const uint8_t* seeds, uint8_t* d_dst) {
    return prove_whole_to_device(ctx, c, w, seeds, d_dst, /*framed=*/true, nullptr, nullptr, nullptr, "rv_prove_batch_device");
}

static int rv_prove_batch_impl(rv_ctx* ctx, const rv_circuit* c, size_t batch, const WitSrc& w, const uint8_t* seeds, const BatchDst& out) {
    LibBusy busy_guard;  // (compile.h: the background unmapper keeps still while the GPU is driven)
    const uint8_t* const wit_gf2 = w.gf2;
    const uint64_t* const wit_z64 = w.z64;
    const size_t n_gf2 = w.n_gf2, n_z64 = w.n_z64;
    uint8_t** const proofs = out.proofs;
    size_t* const proof_lens = out.proof_lens;
    const bool dev = out.d_dst != nullptr;
    if (!ctx || !c || !batch || (dev ? !seeds : (!proofs || !proof_lens))) return RV_E_ARG;
    const Compiled& cc = c->cc;
    for (size_t b = 0; b < batch && !dev; b++) proofs[b] = nullptr, proof_lens[b] = 0;
    if (n_gf2 < cc.n_in || n_z64 < cc.n_in64) return RV_E_WITNESS_SHORT;
    if ((cc.n_in && !wit_gf2) || (cc.n_in64 && !wit_z64)) return RV_E_ARG;
    std::vector<uint8_t> drawn;
    if (!seeds) {
        drawn.resize(batch * RV_TOTAL_REPS * 16);
        if (int rs = os_seeds(drawn.data(), drawn.size())) return rs;
        seeds = drawn.data();
    }
    auto one_by_one = [&]() {  // Z64 / mixed circuits and batches of one: the plain entry point, proof after proof
        for (size_t b = 0; b < batch && dev; b++) {
            int rc = prove_framed_device(ctx, c, w.from(b), seeds + b * RV_TOTAL_REPS * 16, out.d_dst + b * out.stride);
            if (rc) return rc;
        }
        if (dev) return (int)RV_OK;
        for (size_t b = 0; b < batch; b++) {
            int rc = guarded([&]() -> int { return rv_prove_impl(ctx, c, w.from(b), seeds + b * RV_TOTAL_REPS * 16, &proofs[b], &proof_lens[b]); });
            if (rc) {
                for (size_t k = 0; k <= b; k++) rv_free(proofs[k]), proofs[k] = nullptr, proof_lens[k] = 0;
                return rc;
            }
        }
        return (int)RV_OK;
    };
    if (batch == 1) return one_by_one();
    HIPCHK(hipSetDevice(ctx->device));
    const size_t big_gates = batch_big_gates();  // (GF(2) circuits from this many gates on take the proofs-in-flight path)
    // Z64 / mixed circuits take the one-pass path below the same threshold (GF(2) and Z64 gates counted together); large ones
    // prove one by one (the worker threads' path is GF(2)-only: its early corrections would need a 2 GB staging area per worker)
    const bool has64 = !cc.gates64.empty();
    if (has64 && cc.gates.size() + cc.gates64.size() >= big_gates) return one_by_one();
    if (has64) {
        // A pass keeps every proof's working set resident (wmask64 alone is 16 KB per Z64 wire): larger batches run as
        // consecutive chunks of what fits in half of the free device memory (RV_BATCH_MAX caps a chunk), each with its own slab
        size_t free_b = 0, total_b = 0;
        if (hipMemGetInfo(&free_b, &total_b) != hipSuccess) return RV_E_DEVICE;
        const size_t per_proof = cc.info.scratch_bytes + whole_proof_layout(cc).total + cc.n_in + 8 * cc.n_in64 + 4096;
        size_t chunk = std::min<size_t>(std::max<size_t>((free_b + ctx->cached_bytes) / 2 / per_proof, 2), 4096);
        if (const char* e = getenv("RV_BATCH_MAX")) chunk = std::min<size_t>(chunk, (size_t)std::max(atoi(e), 1));
        if (batch > chunk) {
            for (size_t b0 = 0; b0 < batch; b0 += chunk) {
                const int rc = rv_prove_batch_impl(ctx, c, std::min(chunk, batch - b0), w.from(b0), seeds + b0 * RV_TOTAL_REPS * 16,
                                                   dev ? BatchDst{nullptr, nullptr, out.d_dst + b0 * out.stride, out.stride}
                                                       : BatchDst{proofs + b0, proof_lens + b0, nullptr, 0});
                if (rc) {
                    for (size_t k = 0; k < b0 && !dev; k++) rv_free(proofs[k]), proofs[k] = nullptr, proof_lens[k] = 0;
                    return rc;
                }
            }
            return RV_OK;
        }
    }
    // (the device form proves a large circuit's statements one after another: the workers below exist to hide a proof's trip
    // over PCIe behind another proof's kernels, and the device form makes no such trip)
    if (dev && cc.gates.size() >= big_gates) return one_by_one();
    if (cc.gates.size() >= big_gates) {
        // Large circuits fill the GPU on their own; what is left to gain is overlapping one proof's VALU-bound phases
        // (masks, digests) with another's memory-bound interpreter, and a third one's 50 MB trip over PCIe.  A few host
        // threads, each with its own worker context (stream + arena; the circuit's device arrays are shared read-only),
        // prove alternate statements through the ordinary single-proof path.  Host bytes in, host proof bytes out on the
        // 10^7-gate circuit: 6.7 ms for a single rv_prove, 5.9 per proof with two threads, 5.4 with three, 5.5 with four
        // (device-resident proofs: 4.9 with two in flight, no gain from a third).
        constexpr size_t T_MAX = 8;
        static const size_t T = [] {
            const char* e = getenv("RV_BATCH_THREADS");
            return (size_t)std::min(std::max(e ? atoi(e) : 3, 1), (int)T_MAX);
        }();
        // Which hardware queue a stream gets (round 6).  The runtime deals the streams of ONE priority class to four hardware queues --
        // a fifth stream shares the queue of an earlier one -- and streams of different classes never share.  Two ACTIVE streams on one
        // queue (a worker's level launches behind another worker's mask chunks, or behind each other's event waits) cost a batch
        // 1 - 4 ms per proof, and whether that happened used to depend on what else in the process had made streams of the default
        // class before: the caller's context (three), PyTorch (bench.py), earlier calls.  The workers therefore keep out of the default
        // class altogether: worker k's main stream in the HIGHEST class, its mask-generator stream in the LOWEST (the level launches are
        // the latency-bound side, the cipher takes what is left: the same order as s_setprio inside the compute units), no second
        // stream -- three workers = three streams per class, every one on a queue of its own, whatever the rest of the process does.
        // RV_BATCH_CLASSES overrides, two letters per worker (main, masks) out of H / N / L, e.g. "HHNNLL" = round 5's assignment.
        static const std::string classes = [] {
            const char* e = getenv("RV_BATCH_CLASSES");
            return std::string(e ? e : "HLHLHLHLHLHLHLHL");
        }();
        static const int prio_levels = [] {
            int lo = 0, hi = 0;
            if (hipDeviceGetStreamPriorityRange(&lo, &hi) != hipSuccess) lo = hi = 0, (void)hipGetLastError();
            return lo - hi + 1;
        }();
        auto cls = [&](size_t i) {
            const char ch = i < classes.size() ? classes[i] : 'N';
            const int lowest = prio_levels - 1;
            return prio_levels < 2 ? -1 : ch == 'H' ? 0 : ch == 'L' ? lowest : lowest / 2 + (lowest == 1 ? -1 : 0);
        };
        while (ctx->workers.size() < T) {
            rv_ctx* w = nullptr;
            const size_t k = ctx->workers.size();
            int mc = cls(2 * k), kc = cls(2 * k + 1);
            if (mc < 0 && kc >= 0) mc = kc;  // ("N" on a device with two classes: the default priority has no class number of its own)
            int rcw = ctx_create_impl(ctx->device, &w, mc, kc);
            if (rcw) return rcw;
            ctx->workers.push_back(w);
        }
        // every proof of the batch lands in a slice of ONE page-locked buffer (released when the last proof has been
        // rv_free'd): a buffer per proof meant a hipHostMalloc of tens of MB per proof as soon as the caller held more
        // proofs than the pool keeps idle -- 7.7 ms per proof at 16 proofs per call instead of 6.2 at 2
        const size_t stride = (whole_proof_layout(cc).total + 4095) & ~(size_t)4095;
        uint8_t* slab = (uint8_t*)g_pinned.get(std::max<size_t>(stride * batch, PinnedPool::MIN_BYTES));
        if (!slab) return RV_E_NOMEM;
        int rcs[T_MAX] = {};
        std::thread th[T_MAX];
        static const bool big_stats = getenv("RV_BATCH_STATS") != nullptr;
        const auto t_call = std::chrono::steady_clock::now();
        std::vector<std::array<double, 5>> span(batch);
        std::atomic<size_t> next_proof{0};
        for (size_t t = 0; t < T; t++)
            th[t] = std::thread([&, t] {
                try {
                    if (hipSetDevice(ctx->device) != hipSuccess) {
                        rcs[t] = RV_E_DEVICE;
                        return;
                    }
                    // (the next statement nobody has taken: a worker whose queue gets the GPU more often -- the highest class is served
                    // first -- proves more of the batch instead of idling at the end of its fixed share)
                    for (size_t b; rcs[t] == RV_OK && (b = next_proof.fetch_add(1, std::memory_order_relaxed)) < batch;) {
                        span[b][0] = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_call).count();
                        // (GF(2) circuits only: the worker is given no Z64 witness)
                        rcs[t] = rv_prove_impl(ctx->workers[t], c, WitSrc{w.from(b).gf2, n_gf2, w.stride_gf2, nullptr, 0, 0, w.dev},
                                               seeds + b * RV_TOTAL_REPS * 16, &proofs[b], &proof_lens[b], slab + b * stride, stride);
                        span[b][1] = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_call).count();
                        for (int k = 0; k < 3; k++) span[b][2 + k] = g_prove_marks[k];
                        if (big_stats && g_prove_marks[1] > 5.0) {
                            std::string line = "[rv batch] slow host side, proof " + std::to_string(b) + ":";
                            for (auto& m : g_ht.marks) line += std::string(" ") + m.first + " " + std::to_string(m.second).substr(0, 5);
                            fprintf(stderr, "%s\n", line.c_str());
                        }
                    }
                } catch (...) {
                    rcs[t] = RV_E_NOMEM;
                }
            });
        for (size_t t = 0; t < T; t++) th[t].join();
        if (big_stats) {
            fprintf(stderr, "[rv batch] %zu proofs on %zu workers, %.2f ms:", batch, T,
                    std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_call).count());
            for (size_t b = 0; b < batch; b++)
                fprintf(stderr, " %zu[%.1f-%.1f: q %.1f o %.1f s %.1f]", b, span[b][0], span[b][1], span[b][2], span[b][3], span[b][4]);
            fprintf(stderr, "\n");
        }
        for (int r : rcs)
            if (r) {
                for (size_t b = 0; b < batch; b++) proofs[b] = nullptr, proof_lens[b] = 0;
                g_pinned.put(slab);
                return r;
            }
        g_pinned.share(slab, batch);  // from here on the proofs own it
        ctx->prof.calls += batch;
        return RV_OK;
    }
    std::vector<rv_shard*> sh(batch, nullptr);
    std::vector<InterpParams> pp(batch);
    std::vector<Interp64Params> pp64(has64 ? batch : 0);
    InterpParams* d_pp = nullptr;
    int rc = RV_OK;
    uint8_t* staging = nullptr;
    std::vector<void*> pinned_tmp;  // argument blocks of the replayed launches (page-locked, returned at the end)
    std::vector<void*> device_tmp;
    auto cleanup = [&](int code) {
        g_recorder = nullptr;
        (void)hipStreamSynchronize(ctx->stream);
        for (rv_shard* s : sh)
            if (s) {
                s->destroy();
                delete s;
            }
        ctx->release(d_pp);
        for (void* q : device_tmp) ctx->release(q);
        for (void* q : pinned_tmp) g_pinned.put(q);
        if (staging) g_pinned.put(staging);
        if (code && !dev)
            for (size_t b = 0; b < batch; b++) rv_free(proofs[b]), proofs[b] = nullptr, proof_lens[b] = 0;
        return code;
    };
    const uint32_t R = RV_TOTAL_REPS;
    // The per-proof phases are strings of small kernels, the same string with the same grids for every proof of the
    // circuit.  Each proof's string is RECORDED (launch.h) instead of launched, then every step is issued once for the
    // whole batch (gridDim.y = proof, arguments from a device array): 35 launches per batch instead of 35 per proof.
    std::vector<LaunchRecorder> recs(batch);
    for (auto& r : recs) r.batch = (unsigned)batch;
    struct RecorderOff {  // whatever way this function is left (an exception included), launches go to the stream again
        ~RecorderOff() { g_recorder = nullptr; }
    } recorder_off;
    static const bool stats = getenv("RV_BATCH_STATS") != nullptr;
    auto t_last = std::chrono::steady_clock::now();
    auto mark = [&](const char* what) {
        if (!stats) return;
        const auto t = std::chrono::steady_clock::now();
        fprintf(stderr, "[rv batch] %-28s %8.3f ms\n", what, std::chrono::duration<double, std::milli>(t - t_last).count());
        t_last = t;
    };
    auto replay = [&]() -> int { return replay_recorded(ctx, recs, pinned_tmp, device_tmp); };
    // ---- per proof: seeds, witness, keys, masks, buffers.  What the host sends or fetches per proof (seeds, witness,
    // error flag, the proof itself) lives in ONE allocation per kind, a slot per proof, so that it moves in one copy
    // per batch instead of one per proof (1 280 small copies were a fifth of a batch's GPU time).  The slots start
    // 256 bytes into their slab: no proof's pointer equals an arena block, the slabs are released exactly once below.
    constexpr size_t SLAB_HEAD = 256;
    const size_t wit_stride = (std::max<size_t>(cc.n_in, 1) + 15) & ~(size_t)15;
    const size_t out_stride = (whole_proof_layout(cc).total + 4 + 255) & ~(size_t)255;
    uint8_t *d_seeds_all = nullptr, *d_wit_all = nullptr, *d_out_all = nullptr;
    int* d_err_all = nullptr;
    if ((rc = dalloc(ctx, SLAB_HEAD + batch * (size_t)R * 16, &d_seeds_all))) return cleanup(rc);
    device_tmp.push_back(d_seeds_all);
    if ((rc = dalloc(ctx, SLAB_HEAD + batch * wit_stride, &d_wit_all))) return cleanup(rc);
    device_tmp.push_back(d_wit_all);
    if (!dev) {  // (the device form's proofs are written where the caller wants them)
        if ((rc = dalloc(ctx, SLAB_HEAD + batch * out_stride, &d_out_all))) return cleanup(rc);
        device_tmp.push_back(d_out_all);
    }
    if ((rc = dalloc(ctx, SLAB_HEAD / sizeof(int) + batch, &d_err_all))) return cleanup(rc);
    device_tmp.push_back(d_err_all);
    if (hipMemcpyAsync(d_seeds_all + SLAB_HEAD, seeds, batch * (size_t)R * 16, hipMemcpyHostToDevice, ctx->stream) != hipSuccess ||
        (cc.n_in && hipMemcpy2DAsync(d_wit_all + SLAB_HEAD, wit_stride, wit_gf2, w.stride_gf2, cc.n_in, batch, w.kind(),
                                     ctx->stream) != hipSuccess))
        return cleanup(RV_E_DEVICE);
    const size_t wit64_stride = (std::max<size_t>(cc.n_in64, 1) + 1) & ~(size_t)1;  // (u64 words)
    uint64_t* d_wit64_all = nullptr;
    if (has64) {
        if ((rc = dalloc(ctx, SLAB_HEAD / 8 + batch * wit64_stride, &d_wit64_all))) return cleanup(rc);
        device_tmp.push_back(d_wit64_all);
        if (cc.n_in64 && hipMemcpy2DAsync(d_wit64_all + SLAB_HEAD / 8, wit64_stride * 8, wit_z64, w.stride_z64 * 8, cc.n_in64 * 8, batch,
                                          w.kind(), ctx->stream) != hipSuccess)
            return cleanup(RV_E_DEVICE);
    }
    wit_count(w, batch * (cc.n_in + cc.n_in64 * 8));
    for (size_t b = 0; b < batch && !rc; b++) {
        rv_shard* s = sh[b] = new rv_shard();
        s->ctx = ctx;
        s->c = c;
        s->rep_begin = 0;
        s->R = R;
        s->NQ = R / 4;
        s->d_seeds = d_seeds_all + SLAB_HEAD + b * (size_t)R * 16;
        s->d_wit = d_wit_all + SLAB_HEAD + b * wit_stride;
        s->d_err = d_err_all + SLAB_HEAD / sizeof(int) + b;
        if ((rc = dalloc(ctx, (size_t)R * 128, &s->d_keys))) break;
        g_recorder = &recs[b];
        launch_expand_seeds(ctx->stream, s->d_seeds, R, s->d_keys);
        // (a fresh shard's z64f is false, and rv_shard_commit never sets it under a recorder: k_z64_fused, whose mask generator
        // and schedule are per proof, stays out of the batch; the Z64 masks come from the recorded k_aes_z64_masks, the levels
        // from k_interp64_b)
        Interp64Params p64{};
        pp[b] = InterpParams{};
        pp[b].wit = s->d_wit;
        if (!(rc = shard_setup_prg(s, nullptr))) rc = shard_run_alloc(s, pp[b], p64);
        if (has64) {
            p64.wit = d_wit64_all + SLAB_HEAD / 8 + b * wit64_stride;
            pp64[b] = p64;
        }
        g_recorder = nullptr;
    }
    if (rc) return cleanup(rc);
    mark("record setup/masks");
    ctx->phase(RV_PH_MASKS);  // (whole-batch phases: keys + masks, interpreter, digests + openings)
    if ((rc = replay())) return cleanup(rc);
    mark("replay setup/masks");
    // ---- all proofs level by level
    ctx->phase(RV_PH_INTERP);
    if ((rc = dalloc(ctx, batch, &d_pp))) return cleanup(rc);
    if (hipMemcpyAsync(d_pp, pp.data(), batch * sizeof(InterpParams), hipMemcpyHostToDevice, ctx->stream) != hipSuccess) return cleanup(RV_E_DEVICE);
    Interp64Params* d_pp64 = nullptr;
    if (has64) {
        if ((rc = dalloc(ctx, batch, &d_pp64))) return cleanup(rc);
        device_tmp.push_back(d_pp64);
        if (hipMemcpyAsync(d_pp64, pp64.data(), batch * sizeof(Interp64Params), hipMemcpyHostToDevice, ctx->stream) != hipSuccess) return cleanup(RV_E_DEVICE);
    }
    launch_levels_batched(ctx, c, MODE_PROVE, d_pp, d_pp64, batch);
    // (the digests' recording below counts its launches too: the interpreter's phase ends here)
    if (has64) ctx->phase(-1);
    mark("interpreter launches");
    // ---- per proof: digests, commitment + challenge + openings on the device, proof bytes to the host
    size_t slot = 0;
    size_t lens[4] = {0, 0, 0, 0};  // the same for every proof of the circuit (40 / 216 split)
    for (size_t b = 0; b < batch && !rc; b++) {
        rv_shard* s = sh[b];
        OpenArgs a;
        a.dst = dev ? out.d_dst + b * out.stride : d_out_all + SLAB_HEAD + b * out_stride;
        a.framed = true;
        a.no_sync = true;
        OpenResult res;
        g_recorder = &recs[b];
        if (!(rc = shard_run_hash(s)) && !(rc = shard_join(s))) rc = shard_open_impl(s, a, &res);
        g_recorder = nullptr;
        for (int k = 0; k < 4; k++) lens[k] = res.lens[k];
    }
    if (rc) return cleanup(rc);
    mark("record digests/openings");
    ctx->phase(RV_PH_HASH);
    if ((rc = replay())) return cleanup(rc);
    ctx->phase(-1);
    mark("replay digests/openings");
    const size_t total = 32 + 4 * 8 + lens[0] + lens[1] + lens[2] + lens[3];
    if (dev) {
        // the counts on the device, and only the error flags to the host: one copy, one synchronisation
        if (total > out.stride || batch > 0x3FFFFFFFu || !launch_frame_counts(ctx->stream, out.d_dst, out.stride, (uint32_t)batch, lens) ||
            hipGetLastError() != hipSuccess)
            return cleanup(RV_E_DEVICE);
        staging = (uint8_t*)g_pinned.get(std::max<size_t>(batch * sizeof(int), PinnedPool::MIN_BYTES));
        if (!staging) return cleanup(RV_E_NOMEM);
        if (hipMemcpyAsync(staging, d_err_all + SLAB_HEAD / sizeof(int), batch * sizeof(int), hipMemcpyDeviceToHost, ctx->stream) != hipSuccess)
            return cleanup(RV_E_DEVICE);
    } else {
        // one page-locked staging area for the whole batch (a device-to-host copy into pageable memory would block the
        // host until the kernels have run): the proofs at their device stride, then the error flags
        if (total > out_stride) return cleanup(RV_E_DEVICE);
        slot = out_stride;
        staging = (uint8_t*)g_pinned.get(std::max<size_t>(slot * batch + batch * sizeof(int), PinnedPool::MIN_BYTES));
        if (!staging) return cleanup(RV_E_NOMEM);
        if (hipMemcpyAsync(staging, d_out_all + SLAB_HEAD, slot * batch, hipMemcpyDeviceToHost, ctx->stream) != hipSuccess ||
            hipMemcpyAsync(staging + slot * batch, d_err_all + SLAB_HEAD / sizeof(int), batch * sizeof(int), hipMemcpyDeviceToHost,
                           ctx->stream) != hipSuccess)
            return cleanup(RV_E_DEVICE);
        for (size_t b = 0; b < batch; b++) proof_lens[b] = total;
    }
    mark("queue device-to-host copies");
    if (hipStreamSynchronize(ctx->stream) != hipSuccess) return cleanup(hip_fail(hipGetLastError(), "batch sync", __FILE__, __LINE__));
    ctx->collect();
    mark("wait for the GPU");
    for (size_t b = 0; b < batch; b++) {
        int err = 0;
        memcpy(&err, staging + slot * batch + b * sizeof(int), sizeof err);
        if (err) return cleanup(RV_E_WITNESS_INVALID);
    }
    if (!dev) {
        // The proofs are handed out where they landed: slices of the page-locked staging buffer, which returns to the
        // pool when the last of them has been rv_free'd (no second copy into 256 freshly mapped buffers, no 256
        // munmaps in the caller: together they cost more than the GPU work of an AES-128 batch).  RV_BATCH_COPY_OUT=1
        // gives every proof its own malloc'ed buffer instead (callers that keep single proofs of many batches alive).
        static const bool copy_out = getenv("RV_BATCH_COPY_OUT") != nullptr;
        if (copy_out) {
            for (size_t b = 0; b < batch; b++) {
                proofs[b] = (uint8_t*)malloc(proof_lens[b]);
                if (!proofs[b]) return cleanup(RV_E_NOMEM);
                memcpy(proofs[b], staging + b * slot, proof_lens[b]);
            }
        } else {
            g_pinned.share(staging, batch);
            for (size_t b = 0; b < batch; b++) proofs[b] = staging + b * slot;
            staging = nullptr;  // owned by the proofs now
        }
        for (size_t b = 0; b < batch; b++) frame_counts_host(proofs[b], lens);
    }
    ctx->prof.calls += batch;
    mark("copy proofs out");
    rc = cleanup(RV_OK);
    mark("cleanup");
    return rc;
}

extern "C" int rv_prove_batch(rv_ctx* ctx, const rv_circuit* c, size_t batch, const uint8_t* wit_gf2, size_t n_gf2,
                              const uint64_t* wit_z64, size_t n_z64, const uint8_t* seeds, uint8_t** proofs, size_t* proof_lens) {
    return guarded([&] { return rv_prove_batch_impl(ctx, c, batch, wit_host(wit_gf2, n_gf2, wit_z64, n_z64), seeds, BatchDst{proofs, proof_lens, nullptr, 0}); });
}
