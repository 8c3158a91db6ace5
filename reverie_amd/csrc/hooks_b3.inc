// Part of api.hip (#included there after stream.inc: the incremental tree's inc_absorb / inc_finish live there): the transcript-hash
// kernels (b3_tree.hip, z64.hip: k_b3_chunks_contig), one production launch at a time on caller-supplied data.
//
// rv_hook_b3_plan answers which kernel production picks for a shape, on the host alone.  The other hooks upload their inputs, fill every
// output buffer with 0xA5, call the production launch function on the context's stream -- with production's own choice (choice = 0) or
// with a forced one (launch_*_as / *_run: the same launch code production runs after choosing) -- and return the buffers whole: a word
// the launch did not write is still 0xA5A5A5A5.  A forced choice whose kernel does not take the shape is refused with RV_E_ARG before
// anything is allocated or launched, as is every shape whose launch could leave a buffer or the kernel's LDS.
// batch >= 2: the call is recorded `batch` times, on `batch` different inputs laid end to end, into LaunchRecorders whose batch is
// `batch`, and replayed through replay_recorded (batch.inc) -- the launchers see a batch and the bodies run through k_many.
namespace {
constexpr int B3_FILL = 0xA5;
constexpr uint32_t B3_HOOK_MAX_BATCH = 64;
constexpr uint64_t B3_HOOK_MAX_CHUNKS = 1ull << 20;

bool b3_hook_batch_ok(uint32_t batch) { return batch == 0 || (batch >= 2 && batch <= B3_HOOK_MAX_BATCH); }
// strictly ascending quad words below NQ (the verifier's list); no list: n_quads must be 0
bool b3_hook_quads_ok(const uint32_t* quads, uint32_t n_quads, uint32_t NQ) {
    if (!quads) return n_quads == 0;
    if (!n_quads || n_quads > NQ) return false;
    for (uint32_t i = 0; i < n_quads; i++)
        if (quads[i] >= NQ || (i && quads[i] <= quads[i - 1])) return false;
    return true;
}
// issue(b) for the one direct call (batch = 0), or recorded for b = 0 .. batch - 1 and replayed as one batch
template <class F>
int b3_hook_issue(rv_ctx* ctx, uint32_t batch, F&& issue) {
    if (!batch) {
        issue((size_t)0);
        HIPCHK(hipGetLastError());
        return RV_OK;
    }
    std::vector<LaunchRecorder> recs(batch);
    for (uint32_t b = 0; b < batch; b++) {
        recs[b].batch = batch;
        g_recorder = &recs[b];
        issue((size_t)b);
        g_recorder = nullptr;
    }
    std::vector<void*> pinned_tmp, device_tmp;
    int rc = replay_recorded(ctx, recs, pinned_tmp, device_tmp);
    if (hipStreamSynchronize(ctx->stream) != hipSuccess && !rc) rc = RV_E_DEVICE;
    for (void* q : device_tmp) ctx->release(q);
    for (void* q : pinned_tmp) g_pinned.put(q);
    return rc;
}
}  // namespace

// out[13]: [0] the byte-row chunk kernel of an online stream of n_on events (B3ChunkKernel; 0: nothing is launched), [1] the bit-row chunk
// kernel of a preprocessing stream of n_pre events, [2..4] k_b3_reduce<2> launches, nodes at the top and the top kernel (B3TopKernel) of
// the online stream's tree, [5..7] the same of the preprocessing stream's, [8] launch_b3_pair_small (B3PairSmall; 0: not taken),
// [9] b3_pair_big_ok, [10] launch_b3_pair_big's launches and [11], [12] the nodes of the preprocessing / online stream at its shared top
// (0, 0, 0 when not taken).  listed: the online stream with a quad list of n_quads words; batch: the recorder's batch, 0 without one.
extern "C" int rv_hook_b3_plan(uint64_t n_pre, uint64_t n_on, uint32_t NQ, int listed, uint32_t n_quads, uint32_t batch, uint32_t out[13]) {
    if (!out || !NQ || NQ > RV_TOTAL_REPS / 4 || (!listed && n_quads)) return RV_E_ARG;
    const uint64_t c_pre = n_pre == 0 ? 1 : (n_pre + 1023) / 1024, c_on = n_on == 0 ? 1 : (n_on + 1023) / 1024;
    out[0] = b3_choose_stream_chunks(c_on, NQ, listed != 0, n_quads, batch);
    out[1] = b3_choose_bits_chunks(c_pre, NQ, batch);
    const B3TreePlan t_on = b3_plan_tree(c_on, batch), t_pre = b3_plan_tree(c_pre, batch);
    out[2] = t_on.reduces, out[3] = t_on.n_top, out[4] = t_on.top;
    out[5] = t_pre.reduces, out[6] = t_pre.n_top, out[7] = t_pre.top;
    out[8] = b3_choose_pair_small(n_pre, n_on, NQ, listed != 0, n_quads, batch);
    out[9] = b3_pair_big_takes(n_pre, n_on, NQ, listed != 0, n_quads, batch != 0);
    out[10] = out[11] = out[12] = 0;
    if (out[9]) {
        const B3PairBigPlan p = b3_plan_pair_big_tree(c_pre, c_on);
        out[10] = 1 + p.reduces + 1, out[11] = p.top_a, out[12] = p.top_b;
    }
    return RV_OK;
}

// kind 0: byte rows [n][width] u32 (width = NQ); 1: bit rows [n][width / 2] u8; 2: contiguous streams [width][stride_words] u64 of which
// the first n words are hashed (width = R).  -> cvs: per input cv_words words, of which the first n_chunks * R * 8 are the chaining values
// [n_chunks][R][8]; *chosen: the B3ChunkKernel launched (kind 2 has one kernel: choice must be 0)
extern "C" int rv_hook_b3_chunks(rv_ctx* ctx, int kind, const void* stream, uint64_t n, uint32_t width, uint64_t stride_words, const uint32_t* quads,
                                 uint32_t n_quads, uint64_t chunk_base, uint32_t root_ok, uint32_t choice, uint32_t batch, uint32_t* cvs, uint64_t cv_words,
                                 uint32_t* chosen) {
    if (!ctx || !cvs || !chosen || kind < 0 || kind > 2 || choice > B3C_UNI || root_ok > 1 || !b3_hook_batch_ok(batch) || (n && !stream)) return RV_E_ARG;
    const uint64_t n_bytes = kind == 2 ? n * 8 : n;  // (stream bytes per repetition)
    const uint64_t n_chunks = n_bytes == 0 ? 1 : (n_bytes + 1023) / 1024;
    if (n > HOOK_MAX || n_chunks > B3_HOOK_MAX_CHUNKS || chunk_base > ~0ull - n_chunks) return RV_E_ARG;
    const uint32_t R = kind == 2 ? width : width * 4;
    if (kind == 2) {
        if (!R || R > RV_TOTAL_REPS || stride_words < n || stride_words > HOOK_MAX || quads || n_quads || choice) return RV_E_ARG;
    } else {
        if (!width || width > RV_TOTAL_REPS / 4 || (kind == 1 && (width & 1 || quads || n_quads)) || !b3_hook_quads_ok(quads, n_quads, width)) return RV_E_ARG;
        if (choice && !b3_chunk_kernel_takes((B3ChunkKernel)choice, width, quads != nullptr, kind == 1)) return RV_E_ARG;
    }
    if (cv_words < n_chunks * R * 8 || cv_words > HOOK_MAX) return RV_E_ARG;
    HIPCHK(hipSetDevice(ctx->device));
    const size_t B = batch ? batch : 1;
    const size_t in_bytes = kind == 0 ? (size_t)n * width * 4 : kind == 1 ? (size_t)n * (width / 2) : (size_t)R * stride_words * 8;
    HookBufs bufs(ctx);
    uint8_t* d_in = nullptr;
    uint32_t *d_quads = nullptr, *d_cv = nullptr;
    int rc;
    if ((rc = bufs.up((const uint8_t*)stream, B * in_bytes, &d_in)) || (quads && (rc = bufs.up(quads, (size_t)n_quads, &d_quads))) ||
        (rc = bufs.filled(B3_FILL, B * (size_t)cv_words, &d_cv)))
        return rc;
    const uint32_t eff_batch = batch;  // (what b3_batch_now() answers while a call of the batch is recorded)
    B3ChunkKernel k = B3C_NONE;
    if (kind == 0) k = choice ? (B3ChunkKernel)choice : b3_choose_stream_chunks(n_chunks, width, quads != nullptr, n_quads, eff_batch);
    if (kind == 1) k = choice ? (B3ChunkKernel)choice : b3_choose_bits_chunks(n_chunks, width, eff_batch);
    *chosen = k;
    rc = b3_hook_issue(ctx, batch, [&](size_t b) {
        const uint8_t* in = d_in + b * in_bytes;
        uint32_t* cv = d_cv + b * (size_t)cv_words;
        if (kind == 0) {
            if (choice)
                launch_b3_stream_chunks_as(ctx->stream, k, (const uint32_t*)in, n, width, cv, d_quads, n_quads, chunk_base, root_ok);
            else
                launch_b3_stream_chunks(ctx->stream, (const uint32_t*)in, n, width, cv, d_quads, n_quads, chunk_base, root_ok);
        } else if (kind == 1) {
            if (choice)
                launch_b3_stream_bits_chunks_as(ctx->stream, k, in, n, width, cv, chunk_base, root_ok);
            else
                launch_b3_stream_bits_chunks(ctx->stream, in, n, width, cv, chunk_base, root_ok);
        } else {
            launch_b3_contig_chunks(ctx->stream, (const uint64_t*)in, stride_words, n, R, cv, chunk_base, root_ok);
        }
    });
    if (rc) return rc;
    if ((rc = bufs.down(cvs, d_cv, B * (size_t)cv_words))) return rc;
    HIPCHK(hipStreamSynchronize(ctx->stream));
    return RV_OK;
}

// launch_b3_pair_small on a bit-row and a byte-row transcript of NQ quad words: both streams' chaining values (cv_pre_words / cv_on_words
// words per input) and digests (dig_words words per input).  *taken: the B3PairSmall form launched; 0: the launcher declined and
// nothing ran.  choice: a forced form (both streams must fit the 64-node tree top; the quad-of-lanes form is not recordable: no batch)
extern "C" int rv_hook_b3_pair_small(rv_ctx* ctx, const uint8_t* pre, uint64_t n_pre, const uint32_t* on, uint64_t n_on, uint32_t NQ, const uint32_t* quads,
                                     uint32_t n_quads, uint32_t choice, uint32_t batch, uint32_t* cv_pre, uint64_t cv_pre_words, uint32_t* cv_on,
                                     uint64_t cv_on_words, uint32_t* dig_pre, uint32_t* dig_on, uint64_t dig_words, uint32_t* taken) {
    if (!ctx || !cv_pre || !cv_on || !dig_pre || !dig_on || !taken || choice > B3P_LANE || !b3_hook_batch_ok(batch) || (n_pre && !pre) || (n_on && !on)) return RV_E_ARG;
    if (!NQ || NQ & 1 || NQ > RV_TOTAL_REPS / 4 || n_pre > HOOK_MAX || n_on > HOOK_MAX) return RV_E_ARG;
    const bool none_listed = quads && !n_quads;  // (a shard without opened repetitions: production's launcher declines)
    if (none_listed ? choice != 0 : !b3_hook_quads_ok(quads, n_quads, NQ)) return RV_E_ARG;
    const uint64_t c_pre = n_pre == 0 ? 1 : (n_pre + 1023) / 1024, c_on = n_on == 0 ? 1 : (n_on + 1023) / 1024;
    const uint32_t R = NQ * 4;
    if (cv_pre_words < c_pre * R * 8 || cv_on_words < c_on * R * 8 || dig_words < (uint64_t)R * 8 || cv_pre_words > HOOK_MAX || cv_on_words > HOOK_MAX ||
        dig_words > HOOK_MAX)
        return RV_E_ARG;
    if (choice && (c_pre > 64 || c_on > 64 || (choice == B3P_QUAD && batch))) return RV_E_ARG;
    const B3PairSmall form = choice ? (B3PairSmall)choice : b3_choose_pair_small(n_pre, n_on, NQ, quads != nullptr, n_quads, batch);
    *taken = form;
    HIPCHK(hipSetDevice(ctx->device));
    const size_t B = batch ? batch : 1, pre_bytes = (size_t)n_pre * (NQ / 2), on_words = (size_t)n_on * NQ;
    HookBufs bufs(ctx);
    uint8_t* d_pre = nullptr;
    uint32_t *d_on = nullptr, *d_quads = nullptr, *d_cva = nullptr, *d_cvb = nullptr, *d_da = nullptr, *d_db = nullptr;
    int rc;
    if ((rc = bufs.up(pre, B * pre_bytes, &d_pre)) || (rc = bufs.up(on, B * on_words, &d_on)) || (quads && (rc = bufs.up(quads, (size_t)n_quads, &d_quads))) ||
        (rc = bufs.filled(B3_FILL, B * (size_t)cv_pre_words, &d_cva)) || (rc = bufs.filled(B3_FILL, B * (size_t)cv_on_words, &d_cvb)) ||
        (rc = bufs.filled(B3_FILL, B * (size_t)dig_words, &d_da)) || (rc = bufs.filled(B3_FILL, B * (size_t)dig_words, &d_db)))
        return rc;
    if (form != B3P_NONE) {
        bool declined = false;
        rc = b3_hook_issue(ctx, batch, [&](size_t b) {
            const uint8_t* p = d_pre + b * pre_bytes;
            const uint32_t* o = d_on + b * on_words;
            uint32_t *ca = d_cva + b * (size_t)cv_pre_words, *cb = d_cvb + b * (size_t)cv_on_words, *da = d_da + b * (size_t)dig_words, *db = d_db + b * (size_t)dig_words;
            if (choice)
                launch_b3_pair_small_as(ctx->stream, form, p, n_pre, o, n_on, NQ, ca, cb, da, db, d_quads, n_quads);
            else if (!launch_b3_pair_small(ctx->stream, p, n_pre, o, n_on, NQ, ca, cb, da, db, d_quads, n_quads))
                declined = true;
        });
        if (rc) return rc;
        if (declined) return RV_E_DEVICE;  // (the launcher and its own choice function disagree)
    }
    if ((rc = bufs.down(cv_pre, d_cva, B * (size_t)cv_pre_words)) || (rc = bufs.down(cv_on, d_cvb, B * (size_t)cv_on_words)) ||
        (rc = bufs.down(dig_pre, d_da, B * (size_t)dig_words)) || (rc = bufs.down(dig_on, d_db, B * (size_t)dig_words)))
        return rc;
    HIPCHK(hipStreamSynchronize(ctx->stream));
    return RV_OK;
}

// launch_b3_pair_big's chunk launch (full rows: NQ = 64) at any number of events; the kernel (k_b3_chunks_pair_uni<0|1|2>) follows from
// the quad list as in production.  (Never recorded: a batch of proofs does not take the shared launches.)
extern "C" int rv_hook_b3_pair_big_chunks(rv_ctx* ctx, const uint8_t* pre, uint64_t n_pre, const uint32_t* on, uint64_t n_on, const uint32_t* quads, uint32_t n_quads,
                                          uint32_t* cv_pre, uint64_t cv_pre_words, uint32_t* cv_on, uint64_t cv_on_words) {
    const uint32_t NQ = 64, R = 256;
    if (!ctx || !cv_pre || !cv_on || (n_pre && !pre) || (n_on && !on) || n_pre > HOOK_MAX || n_on > HOOK_MAX || !b3_hook_quads_ok(quads, n_quads, NQ)) return RV_E_ARG;
    const uint64_t c_pre = n_pre == 0 ? 1 : (n_pre + 1023) / 1024, c_on = n_on == 0 ? 1 : (n_on + 1023) / 1024;
    if (c_pre > B3_HOOK_MAX_CHUNKS || c_on > B3_HOOK_MAX_CHUNKS || cv_pre_words < c_pre * R * 8 || cv_on_words < c_on * R * 8 || cv_pre_words > HOOK_MAX ||
        cv_on_words > HOOK_MAX)
        return RV_E_ARG;
    HIPCHK(hipSetDevice(ctx->device));
    HookBufs bufs(ctx);
    uint8_t* d_pre = nullptr;
    uint32_t *d_on = nullptr, *d_quads = nullptr, *d_cva = nullptr, *d_cvb = nullptr;
    int rc;
    if ((rc = bufs.up(pre, (size_t)n_pre * (NQ / 2), &d_pre)) || (rc = bufs.up(on, (size_t)n_on * NQ, &d_on)) || (quads && (rc = bufs.up(quads, (size_t)n_quads, &d_quads))) ||
        (rc = bufs.filled(B3_FILL, (size_t)cv_pre_words, &d_cva)) || (rc = bufs.filled(B3_FILL, (size_t)cv_on_words, &d_cvb)))
        return rc;
    launch_b3_pair_big_chunks(ctx->stream, d_pre, n_pre, d_on, n_on, d_cva, d_cvb, d_quads, n_quads);
    HIPCHK(hipGetLastError());
    if ((rc = bufs.down(cv_pre, d_cva, (size_t)cv_pre_words)) || (rc = bufs.down(cv_on, d_cvb, (size_t)cv_on_words))) return rc;
    HIPCHK(hipStreamSynchronize(ctx->stream));
    return RV_OK;
}

// b3_reduce_tree over cvs [n][R][8] -> digest (dig_words words per input, the first R * 8 the roots).  choice: a forced B3TopKernel for
// the nodes the reductions leave; plan[3]: reductions launched, nodes at the top, the top kernel
extern "C" int rv_hook_b3_tree(rv_ctx* ctx, const uint32_t* cvs, uint64_t n, uint32_t R, uint32_t choice, uint32_t batch, uint32_t* digest, uint64_t dig_words,
                               uint32_t plan_out[3]) {
    if (!ctx || !cvs || !digest || !plan_out || !n || n > B3_HOOK_MAX_CHUNKS || !R || R > RV_TOTAL_REPS || choice > B3T_TAIL512 || !b3_hook_batch_ok(batch)) return RV_E_ARG;
    if (dig_words < (uint64_t)R * 8 || dig_words > HOOK_MAX) return RV_E_ARG;
    B3TreePlan plan = b3_plan_tree(n, batch);
    if (choice) {
        if (!b3_top_takes((B3TopKernel)choice, plan.n_top)) return RV_E_ARG;
        plan.top = (B3TopKernel)choice;
    }
    plan_out[0] = plan.reduces, plan_out[1] = plan.n_top, plan_out[2] = plan.top;
    HIPCHK(hipSetDevice(ctx->device));
    const size_t B = batch ? batch : 1, words = b3_stream_scratch_words(n * 1024, R);
    HookBufs bufs(ctx);
    uint32_t *d_cur = nullptr, *d_nxt = nullptr, *d_dig = nullptr;
    int rc;
    if ((rc = bufs.up(cvs, B * words, &d_cur)) || (rc = bufs.filled(B3_FILL, B * words, &d_nxt)) || (rc = bufs.filled(B3_FILL, B * (size_t)dig_words, &d_dig))) return rc;
    rc = b3_hook_issue(ctx, batch, [&](size_t b) {
        if (choice)
            b3_reduce_tree_run(ctx->stream, plan, d_cur + b * words, d_nxt + b * words, n, R, d_dig + b * (size_t)dig_words);
        else
            b3_reduce_tree(ctx->stream, d_cur + b * words, d_nxt + b * words, n, R, d_dig + b * (size_t)dig_words);
    });
    if (rc) return rc;
    if ((rc = bufs.down(digest, d_dig, B * (size_t)dig_words))) return rc;
    HIPCHK(hipStreamSynchronize(ctx->stream));
    return RV_OK;
}

// launch_b3_pair_big's tree part: two trees over cvs_a [n_a][R][8] and cvs_b [n_b][R][8] in shared launches, each stream with a ping-pong
// pair of b3_stream_scratch_words as in production -> two digests (dig_words words each), *launches
extern "C" int rv_hook_b3_pair_big_tree(rv_ctx* ctx, const uint32_t* cvs_a, uint64_t n_a, const uint32_t* cvs_b, uint64_t n_b, uint32_t R, uint32_t* dig_a,
                                        uint32_t* dig_b, uint64_t dig_words, uint32_t* launches) {
    if (!ctx || !cvs_a || !cvs_b || !dig_a || !dig_b || !launches || !n_a || !n_b || n_a > B3_HOOK_MAX_CHUNKS || n_b > B3_HOOK_MAX_CHUNKS || !R || R > RV_TOTAL_REPS)
        return RV_E_ARG;
    if (dig_words < (uint64_t)R * 8 || dig_words > HOOK_MAX) return RV_E_ARG;
    HIPCHK(hipSetDevice(ctx->device));
    const size_t wa = b3_stream_scratch_words(n_a * 1024, R), wb = b3_stream_scratch_words(n_b * 1024, R);
    HookBufs bufs(ctx);
    uint32_t *a0 = nullptr, *a1 = nullptr, *b0 = nullptr, *b1 = nullptr, *d_da = nullptr, *d_db = nullptr;
    int rc;
    if ((rc = bufs.up(cvs_a, wa, &a0)) || (rc = bufs.filled(B3_FILL, wa, &a1)) || (rc = bufs.up(cvs_b, wb, &b0)) || (rc = bufs.filled(B3_FILL, wb, &b1)) ||
        (rc = bufs.filled(B3_FILL, (size_t)dig_words, &d_da)) || (rc = bufs.filled(B3_FILL, (size_t)dig_words, &d_db)))
        return rc;
    *launches = launch_b3_pair_big_tree(ctx->stream, a0, a1, n_a, b0, b1, n_b, R, d_da, d_db);
    HIPCHK(hipGetLastError());
    if ((rc = bufs.down(dig_a, d_da, (size_t)dig_words)) || (rc = bufs.down(dig_b, d_db, (size_t)dig_words))) return rc;
    HIPCHK(hipStreamSynchronize(ctx->stream));
    return RV_OK;
}

// The streaming prover's incremental tree over B streams of n chaining values each (cvs [B][n][R][8]): the first n - 1 arrive in
// n_pieces pieces (pieces[] sums to n - 1; each piece one inc_absorb over all B streams -- B = 1: launch_b3_pairs, else
// launch_b3_pairs_batched, 32 streams a launch), the last value closes every stream through inc_finish -> digest (dig_words words each)
extern "C" int rv_hook_b3_incremental(rv_ctx* ctx, const uint32_t* cvs, uint64_t n, uint32_t R, uint32_t B, const uint64_t* pieces, uint32_t n_pieces,
                                      uint32_t* digest, uint64_t dig_words) {
    if (!ctx || !cvs || !digest || !n || n > B3_HOOK_MAX_CHUNKS || !R || R > RV_TOTAL_REPS || !B || B > B3_HOOK_MAX_BATCH || (n_pieces && !pieces)) return RV_E_ARG;
    if (dig_words < (uint64_t)R * 8 || dig_words > HOOK_MAX) return RV_E_ARG;
    uint64_t sum = 0;
    for (uint32_t i = 0; i < n_pieces; i++) {
        if (pieces[i] > n - 1 - sum) return RV_E_ARG;
        sum += pieces[i];
    }
    if (sum != n - 1) return RV_E_ARG;
    HIPCHK(hipSetDevice(ctx->device));
    const size_t words = (size_t)n * R * 8;
    HookBufs bufs(ctx);
    uint32_t *d_cv = nullptr, *d_dig = nullptr;
    int rc;
    if ((rc = bufs.up(cvs, (size_t)B * words, &d_cv)) || (rc = bufs.filled(B3_FILL, (size_t)B * dig_words, &d_dig))) return rc;
    std::vector<IncHash> H(B);
    std::vector<IncHash*> Hs;
    for (IncHash& h : H) Hs.push_back(&h);
    uint64_t at = 0;
    for (uint32_t i = 0; i < n_pieces && !rc; i++) {
        std::vector<uint32_t*> in;
        for (uint32_t b = 0; b < B; b++) in.push_back(d_cv + b * words + (size_t)at * R * 8);
        rc = inc_absorb(ctx, Hs, in, pieces[i], R);
        at += pieces[i];
    }
    for (uint32_t b = 0; b < B && !rc; b++) inc_finish(ctx, H[b], d_cv + b * words + (size_t)(n - 1) * R * 8, R, d_dig + b * (size_t)dig_words);
    if (!rc && hipGetLastError() != hipSuccess) rc = RV_E_DEVICE;
    if (!rc) rc = bufs.down(digest, d_dig, (size_t)B * dig_words);
    if (hipStreamSynchronize(ctx->stream) != hipSuccess && !rc) rc = RV_E_DEVICE;
    for (IncHash& h : H)
        for (uint32_t* p : h.node) ctx->release(p);
    return rc;
}

// launch_join: digs [4][R][8] (pre2, on2, pre64, on64) -> h (h_bytes bytes per input, the first 32 R the joined digests)
extern "C" int rv_hook_b3_join(rv_ctx* ctx, const uint32_t* digs, uint32_t R, uint32_t batch, uint8_t* h, uint64_t h_bytes) {
    if (!ctx || !digs || !h || !R || R > RV_TOTAL_REPS || !b3_hook_batch_ok(batch) || h_bytes < (uint64_t)R * 32 || h_bytes > HOOK_MAX) return RV_E_ARG;
    HIPCHK(hipSetDevice(ctx->device));
    const size_t B = batch ? batch : 1, DW = (size_t)R * 8;
    HookBufs bufs(ctx);
    uint32_t* d_in = nullptr;
    uint8_t* d_h = nullptr;
    int rc;
    if ((rc = bufs.up(digs, B * 4 * DW, &d_in)) || (rc = bufs.filled(B3_FILL, B * (size_t)h_bytes, &d_h))) return rc;
    rc = b3_hook_issue(ctx, batch, [&](size_t b) {
        const uint32_t* in = d_in + b * 4 * DW;
        launch_join(ctx->stream, in, in + DW, in + 2 * DW, in + 3 * DW, R, d_h + b * (size_t)h_bytes);
    });
    if (rc) return rc;
    if ((rc = bufs.down(h, d_h, B * (size_t)h_bytes))) return rc;
    HIPCHK(hipStreamSynchronize(ctx->stream));
    return RV_OK;
}
