// Streaming (bounded-memory) prover -- part of api.hip's translation unit.
//
// The reference's README promises "a streaming interface" on top of its single-pass just-in-time preprocessing
// (/root/reference/README.md:14,38; generator/share.rs:54-65 produces masks on demand, proof/mod.rs:150-152 walks the
// gate list once); the surveyed source version keeps every reconstruction and correction of all 256 repetitions until
// the challenge (transcript/prover.rs:29-31,211,217), which is what limits it on large circuits (SURVEY §5).
//
// Here the gate stream arrives in chunks and the device holds, besides one chunk's working set,
//   * the wire store: one share row + corr bits per GF(2) wire INDEX, one slot per Z64 wire index (the reference's own
//     `wires` vectors, interpreter/single.rs:14-23 -- bounded by wire_counts, not by the number of gates),
//   * per transcript stream an incremental BLAKE3 tree (at most one pending subtree root per level) and the
//     unhashed tail of the stream (< one 1 KiB BLAKE3 chunk per repetition),
//   * the proof being assembled (pass 2).
// Pass 1 (rv_stream_feed ... rv_stream_commit) computes the 256 per-repetition commitments and the Fiat-Shamir
// challenge without keeping any transcript; pass 2 (the same chunks fed again, rv_stream_finish) re-runs the
// interpreter and extracts the openings of the 40 challenged repetitions chunk by chunk (SURVEY §7 "transcript
// retention": re-run instead of store).  The result is byte-identical to rv_prove's.

namespace {

struct IncHash {  // incremental BLAKE3 tree over R per-repetition streams
    uint64_t chunks = 0;           // complete chunks absorbed so far
    std::vector<uint32_t*> node;   // node[l]: [R][8] root of a complete 2^l-chunk subtree (valid when full[l])
    std::vector<char> full;
};

struct StreamTotals {
    uint64_t n_ops = 0, ops_hash = 0;
    uint64_t wit_hash = 0;            // position-keyed digest of the witness elements consumed so far (pass 2 must feed pass 1's)
    uint64_t masks = 0, masks64 = 0;  // ShareGen::next() calls
    uint64_t n_on = 0, n_pre = 0, n_rec = 0, n_in = 0;
    uint64_t on_words64 = 0, pre_words64 = 0, n_rec64 = 0, n_corr64 = 0, n_in64 = 0;
    uint64_t levels = 0, chunks = 0;
    bool operator==(const StreamTotals& o) const {
        return n_ops == o.n_ops && ops_hash == o.ops_hash && wit_hash == o.wit_hash && masks == o.masks && masks64 == o.masks64 && n_on == o.n_on && n_pre == o.n_pre &&
               n_rec == o.n_rec && n_in == o.n_in && on_words64 == o.on_words64 && pre_words64 == o.pre_words64 && n_rec64 == o.n_rec64 &&
               n_corr64 == o.n_corr64 && n_in64 == o.n_in64;
    }
};

}  // namespace

// rv_hook_stream_traffic, counted where the streams queue their copies: witness bytes sent host-to-device, witness bytes taken from
// device memory, proof bytes copied device-to-host at finish, proof bytes copied host-to-device at a verifier's begin
static std::atomic<uint64_t> g_stream_traffic[4];
static void stream_traffic(int k, uint64_t bytes) { g_stream_traffic[k].fetch_add(bytes, std::memory_order_relaxed); }

// up to 24 small device-to-device copies as ONE launch (the pending rows of pass 2: up to 7 + 7 single rows and three short runs per chunk
// were as many hipMemcpyAsync calls, ~5 us of GPU time and a launch each).  Sizes in bytes, multiples of 4; src and dst do not overlap.
struct CopySegs {
    static constexpr int MAX = 24;
    const void* src[MAX];
    void* dst[MAX];
    uint32_t bytes[MAX];
    uint32_t n;
    void add(const void* s, void* d, size_t b) {
        if (!b) return;
        src[n] = s, dst[n] = d, bytes[n] = (uint32_t)b;
        n++;
    }
};
__global__ void k_copy_segs(CopySegs cs) {
    const uint32_t* s = (const uint32_t*)cs.src[blockIdx.x];
    uint32_t* d = (uint32_t*)cs.dst[blockIdx.x];
    const uint32_t n = cs.bytes[blockIdx.x] / 4;
    for (uint32_t i = threadIdx.x; i < n; i += blockDim.x) d[i] = s[i];
}
static void launch_copy_segs(hipStream_t st, const CopySegs& cs) {
    if (cs.n) hipLaunchKernelGGL(k_copy_segs, dim3(cs.n), dim3(256), 0, st, cs);
}

// A batch stream's small copies of one step, for every proof at once: up to 64 strided segments (rows x row_bytes, own pitches) per
// launch, blockIdx.y = segment.  The tails carried in front of a chunk and out of it, the trees' odd nodes, the pending opening rows:
// per proof they were a hipMemcpy(2D)Async or a k_copy_segs launch each.  Sizes and pitches are multiples of 4 bytes; src and dst of
// a launch do not overlap.
struct CopyRows {
    static constexpr uint32_t MAX = 64;
    const uint8_t* src[MAX];
    uint8_t* dst[MAX];
    uint64_t spitch[MAX], dpitch[MAX];
    uint32_t row_bytes[MAX], rows[MAX];
    uint32_t n;
};
__global__ __launch_bounds__(256) void k_copy_rows_batched(CopyRows L) {
    const uint32_t y = blockIdx.y;
    const uint32_t wpr = L.row_bytes[y] / 4;
    const uint64_t total = (uint64_t)wpr * L.rows[y];
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (uint64_t)gridDim.x * blockDim.x) {
        const uint64_t row = i / wpr, w = i % wpr;
        ((uint32_t*)(L.dst[y] + row * L.dpitch[y]))[w] = ((const uint32_t*)(L.src[y] + row * L.spitch[y]))[w];
    }
}
// The small device-to-device copies of one step.  A batch stream collects them and flush() launches them together; a single stream
// (direct) issues every add at once as the call it always was: hipMemcpyAsync for a contiguous run, hipMemcpy2DAsync for a strided
// one, k_copy_segs for a CopySegs.  The first failure of a direct copy stays in `err`.
struct CopyBatch {
    hipStream_t st;
    bool direct;
    hipError_t err = hipSuccess;
    CopyRows L{};
    CopyBatch(hipStream_t s, bool direct_) : st(s), direct(direct_) {}
    void add(void* dst, uint64_t dpitch, const void* src, uint64_t spitch, uint64_t row_bytes, uint64_t rows) {
        if (!row_bytes || !rows) return;
        if (direct) {
            const hipError_t e = rows == 1 ? hipMemcpyAsync(dst, src, row_bytes, hipMemcpyDeviceToDevice, st)
                                           : hipMemcpy2DAsync(dst, dpitch, src, spitch, row_bytes, rows, hipMemcpyDeviceToDevice, st);
            if (err == hipSuccess) err = e;
            return;
        }
        if (L.n == CopyRows::MAX) flush();
        const uint32_t k = L.n++;
        L.src[k] = (const uint8_t*)src, L.dst[k] = (uint8_t*)dst, L.spitch[k] = spitch, L.dpitch[k] = dpitch;
        L.row_bytes[k] = (uint32_t)row_bytes, L.rows[k] = (uint32_t)rows;
    }
    void add(void* dst, const void* src, uint64_t bytes) { add(dst, bytes, src, bytes, bytes, 1); }
    void add(const CopySegs& cs) {
        if (direct) return launch_copy_segs(st, cs);
        for (uint32_t i = 0; i < cs.n; i++) add(cs.dst[i], cs.src[i], cs.bytes[i]);
    }
    void flush() {
        if (L.n) hipLaunchKernelGGL(k_copy_rows_batched, dim3(16, L.n), dim3(256), 0, st, L);
        L.n = 0;
    }
    // flush, and the code of the step's copies
    int finish(const char* what) {
        flush();
        return err == hipSuccess ? RV_OK : hip_fail(err, what, __FILE__, __LINE__);
    }
};

// The four transcript streams of a repetition -- GF(2) preprocessing / online, Z64 preprocessing / online -- in the order of
// rv_stream::d_dig's slots.  What tells them apart is in TR_KIND; everything else treats them alike.
enum { TR_PRE = 0, TR_ON = 1, TR_PRE64 = 2, TR_ON64 = 3, TR_KINDS = 4 };
struct TranscriptKind {
    uint32_t unit;      // events per 1 KiB BLAKE3 chunk
    uint32_t ev_bytes;  // bytes of one event: a row over all repetitions (GF(2)) or one repetition's word (Z64)
    bool per_rep;       // a buffer is [R][pitch] words, one row per repetition (Z64; the tail: [R][128]); else one row per event ([1024][ev_bytes])
    // chaining values of the first n events of a buffer (pitch: a per-repetition buffer's words per row)
    void (*hash)(hipStream_t st, const void* buf, uint64_t pitch, uint64_t n, uint32_t* cvs, uint64_t chunk_base, uint32_t root_ok);
    uint64_t tail_bytes() const { return (uint64_t)(per_rep ? RV_TOTAL_REPS : 1) * unit * ev_bytes; }
    // of `total` events, those that stay unhashed: the last, possibly incomplete chunk -- at least one event stays behind
    uint64_t tail_of(uint64_t total) const { return total ? total - (total - 1) / unit * unit : 0; }
    // n events from the front of src to the front of dst (pitches in words, per-repetition kinds only)
    void copy(CopyBatch& cp, void* dst, uint64_t dpitch, const void* src, uint64_t spitch, uint64_t n) const {
        if (per_rep)
            cp.add(dst, dpitch * 8, src, spitch * 8, n * 8, RV_TOTAL_REPS);
        else
            cp.add(dst, src, n * ev_bytes);
    }
};
static const TranscriptKind TR_KIND[TR_KINDS] = {
    {1024, RV_TOTAL_REPS / 8, false,
     [](hipStream_t st, const void* b, uint64_t, uint64_t n, uint32_t* cvs, uint64_t base, uint32_t root) {
         launch_b3_stream_bits_chunks(st, (const uint8_t*)b, n, RV_TOTAL_REPS / 4, cvs, base, root);
     }},
    {1024, RV_TOTAL_REPS, false,
     [](hipStream_t st, const void* b, uint64_t, uint64_t n, uint32_t* cvs, uint64_t base, uint32_t root) {
         launch_b3_stream_chunks(st, (const uint32_t*)b, n, RV_TOTAL_REPS / 4, cvs, nullptr, 0, base, root);
     }},
    {128, 8, true,
     [](hipStream_t st, const void* b, uint64_t pitch, uint64_t n, uint32_t* cvs, uint64_t base, uint32_t root) {
         launch_b3_contig_chunks(st, (const uint64_t*)b, pitch, n, RV_TOTAL_REPS, cvs, base, root);
     }},
    {128, 8, true,
     [](hipStream_t st, const void* b, uint64_t pitch, uint64_t n, uint32_t* cvs, uint64_t base, uint32_t root) {
         launch_b3_contig_chunks(st, (const uint64_t*)b, pitch, n, RV_TOTAL_REPS, cvs, base, root);
     }},
};
// the carried events of the four streams as a chunk's compile takes them
static void set_carried(ChunkStart& cs, uint64_t pre, uint64_t on, uint64_t pre64, uint64_t on64) {
    cs.pre0 = pre, cs.on0 = on, cs.pre_words64_0 = pre64, cs.on_words64_0 = on64;
}
static bool same_carried(const ChunkStart& a, const ChunkStart& b) {
    return a.on0 == b.on0 && a.pre0 == b.pre0 && a.on_words64_0 == b.on_words64_0 && a.pre_words64_0 == b.pre_words64_0;
}
// (unsigned differences: the 32-bit fields of the arrays wrap the same way)
static void relocate_to(Compiled& cc, const ChunkStart& from, const ChunkStart& to) {
    relocate_chunk(cc, to.on0 - from.on0, to.pre0 - from.pre0, to.on_words64_0 - from.on_words64_0, to.pre_words64_0 - from.pre_words64_0);
}

struct rv_stream {
    rv_ctx* ctx = nullptr;
    size_t z64_wires = 0, gf2_wires = 0;
    static constexpr uint32_t R = RV_TOTAL_REPS, NQ = RV_TOTAL_REPS / 4;
    int pass = 1;
    int sticky = RV_OK;  // first error: the stream is dead afterwards
    // rv_stream_set_compile_flags (the context's when the stream began): RV_COMPILE_DEVICE = every all-GF(2) piece (with
    // RV_COMPILE_DEVICE_Z64: every piece without a B2A op; with RV_COMPILE_DEVICE_B2A as well: every piece) is compiled by the
    // chunk-mode device compiler, on the context's stream right before it runs; what that hands back is compiled on the host
    uint32_t compile_flags = 0;
    bool fed = false;  // a feed has begun: the flags are fixed
    size_t max_chunk_ops = (size_t)1 << 18;  // (10^7-gate circuit: 179 ms with 2^18, 233 ms with 2^20: a piece is compiled by one thread)
    // per-stream device state
    uint8_t *d_seeds = nullptr, *d_keys = nullptr, *d_rkbytes = nullptr;
    uint32_t* d_rk = nullptr;
    uint32_t* d_rows = nullptr;  // [rows_cap][NQ]: carried wire rows first, then the chunk's PRG and computed rows
    uint8_t* d_corr = nullptr;   // [rows_cap][NQ/2]
    size_t rows_cap = 0;
    uint64_t *d_wmask64 = nullptr, *d_wcorr64 = nullptr;  // [ssa64_cap][R*8], [ssa64_cap][R]
    size_t ssa64_cap = 0;
    int* d_err = nullptr;   // OR of the chunks' error flags since the pass began (the chunks' k_shard_init clears d_err0, not this)
    int* d_err0 = nullptr;
    bool unsettled = false;  // chunks were issued without a wait: stream_feed_settle reads d_err behind them
    StreamTotals run, tot;  // running counters of the current pass / totals of pass 1
    // The witness digest of the chunks whose witnesses were fed from device memory (rv_stream_feed_wdev): k_wit_sums adds into
    // *d_wit_sum, and run.wit_hash is the host sum plus this word -- read at commit in the copy commit waits for anyway, and once at
    // finish.  Allocated and cleared by the stream's first such chunk (a host-fed stream never has it), cleared again where commit
    // resets the pass.
    uint64_t* d_wit_sum = nullptr;
    bool wit_dev_pass = false;  // a chunk of the current pass added to *d_wit_sum
    // pass 1: per transcript stream (TR_PRE .. TR_ON64) the incremental tree and the unhashed tail: the events of the last, incomplete
    // BLAKE3 chunk -- [1024][NQ/2] bytes, [1024][NQ] u32, [R][128] u64 twice (TR_KIND)
    struct Transcript {
        IncHash tree;
        uint8_t* d_tail = nullptr;
        uint64_t tail = 0;  // events in d_tail
    };
    Transcript tr[TR_KINDS];
    uint32_t* d_dig = nullptr;  // [4][R][8]
    uint8_t* d_h = nullptr;     // [R][32]
    // pass 2
    OpenLayout L{};
    uint8_t comm[32] = {0}, omit[RV_TOTAL_REPS] = {0};
    std::vector<uint64_t> offs;  // [8][R] record / vector offsets inside the proof (k_fs_challenge)
    OnlineList ol{};
    uint8_t* d_omit = nullptr;   // [R] + Fiat-Shamir tail
    uint64_t* d_offs = nullptr;
    uint8_t* d_proof = nullptr;
    uint32_t* d_pend_rec = nullptr;  // [8][NQ] online rows of reconstructions / inputs not yet packed (fewer than 8 each)
    uint32_t* d_pend_in = nullptr;
    uint8_t* d_pend_pre = nullptr;   // [8][NQ/2]
    uint32_t pend_rec = 0, pend_in = 0, pend_pre = 0;
    uint64_t peak_bytes = 0;  // largest chunk working set seen (diagnostics)
    // pass 3 = the streaming VERIFIER (rv_stream_verify_begin): one pass, the chunks run in verify mode against the proof
    const uint8_t* h_proof = nullptr;  // the caller's proof bytes (must outlive the stream)
    // rv_stream_verify_begin_device, the in-place path: d_vproof is the CALLER's buffer (not released here), no host copy of the proof
    // exists, and finish decides from what the walk brought: comm and the 80 omit bytes of the online records
    bool proof_in_place = false;
    uint8_t dev_comm[32] = {0}, dev_rec_omit[2 * RV_ONLINE_REPS] = {0};
    std::vector<uint8_t> own_proof;    // ... its fallback: the host copy h_proof points to
    size_t proof_len = 0;
    bool format_bad = false;           // wrong repetition counts: the answer is `false` (proof/mod.rs:225-230), nothing runs
    int dev_flags = 0;                 // RV_DEV_ZERO_CHECK of the chunks so far
    uint8_t *d_vproof = nullptr, *d_omit_v = nullptr, *d_omit64_v = nullptr, *d_hco = nullptr, *d_hco64 = nullptr;
    uint32_t *d_keep = nullptr, *d_keep64 = nullptr, *d_onm = nullptr, *d_rk64 = nullptr;
    uint32_t sup_nq = 0, sup_r = 0;  // verifier: quad words / repetitions per row of the supplied-value arrays (InterpParams::sup_nq, Interp64Params::sup_r)
    uint64_t* d_src = nullptr;         // [6][R]: rec off, len; corr off, len; in off, len (bytes inside the proof)
    std::vector<uint64_t> src64;       // the same for the Z64 vectors (shifted per chunk on the host)
    std::vector<uint64_t> src64c;      // ... as the current chunk's copy reads them (lives until the chunk's final synchronisation)
    // pass 1's compiled chunks, kept on the host for pass 2 while they fit RV_STREAM_CACHE_MB (default 1024): a chunk that
    // is fed again with the same cut only needs its transcript offsets moved (relocate_chunk), not a second compile
    struct CachedPiece {
        uint64_t n_ops = 0, digest = 0;
        ChunkStart at;  // the offsets its arrays currently carry
        Compiled cc;
    };
    std::map<uint64_t, CachedPiece> cache;  // by the index of the piece's first op in the stream
    uint64_t cache_bytes = 0;
    // pass 1's TRANSCRIPTS of the stream's LAST chunks, kept on the device for pass 2 while they fit RV_STREAM_KEEP_MB (default: an
    // eighth of the device's memory, at most 32 GiB; 0 = keep nothing): pass 2 takes the openings of such a chunk from them -- no
    // masks, no interpreter, no gate upload a second time.  Only for a stream whose caller promised to feed pass 2 in pass 1's
    // pieces (rv_stream_same_cuts; rv_prove_streaming does): a chunk that RUNS in pass 2 needs the wire store as the chunks before it
    // left it, so every chunk before it must have run too -- the kept chunks are a suffix of the stream (when the budget is full
    // the oldest one goes), and a chunk that has to run after one that did not is an error (RV_E_ARG).  The device memory of a long
    // stream stays bounded: wire store + one chunk + the proof + this budget.
    struct Kept {
        uint64_t n_ops = 0, digest = 0;
        void *on_base = nullptr, *pre_base = nullptr;  // allocations (headroom in front: pass 2 carries up to 14 / 7 pending rows there)
        uint32_t* d_on = nullptr;                      // the chunk's buffers as pass 1 saw them ...
        uint8_t* d_pre = nullptr;
        uint64_t *d_on64 = nullptr, *d_pre64 = nullptr;
        uint64_t on0 = 0, pre0 = 0, on64_0 = 0, pre64_0 = 0;  // ... with that many carried events in front of the chunk's own
        uint64_t onw = 1, prew = 1;                           // pitch of the Z64 buffers
        uint64_t bytes = 0;
    };
    std::map<uint64_t, Kept> kept;  // by the index of the chunk's first op (main thread only)
    uint64_t kept_bytes = 0, kept_peak = 0, keep_cap = 0;
    struct FeedCounts {  // pass 1's per-piece mask / event counts of a multi-piece feed, by the index of the feed's first op
        std::vector<size_t> cut;
        std::vector<uint64_t> cm2, cm64;
        std::vector<StreamEvents> cev;
    };
    std::map<uint64_t, FeedCounts> feed_counts;
    bool same_cuts = false;   // rv_stream_same_cuts
    bool p2_skipped = false;  // pass 2: a chunk was served from kept transcripts (the wire store is stale from there on)
    // A BATCH stream (rv_stream_begin_batch / rv_stream_verify_begin_batch with batch > 1) is a handle over `bat`: one complete
    // single-proof stream per witness / proof, none of which is the handle.  The handle holds no device memory; a feed compiles each
    // chunk once (on the first member that runs: its cache, its counts) and issues the chunk for every member (ChunkRun).
    std::vector<rv_stream*> bat;
    // the proofs a feed runs for: the stream itself, or the batch's members (a verifier's members with a malformed proof run nothing)
    std::vector<rv_stream*> running() {
        if (bat.empty()) return format_bad ? std::vector<rv_stream*>() : std::vector<rv_stream*>{this};
        std::vector<rv_stream*> v;
        for (rv_stream* m : bat)
            if (!m->format_bad) v.push_back(m);
        return v;
    }
    void release_kept(Kept& k) {
        ctx->release(k.on_base);
        ctx->release(k.pre_base);
        ctx->release(k.d_on64);
        ctx->release(k.d_pre64);
        kept_bytes -= std::min(kept_bytes, k.bytes);
        k = Kept();
    }
    static uint64_t compiled_bytes(const Compiled& cc) {
        return cc.gates.capacity() * sizeof(Gate) + cc.gates64.capacity() * sizeof(Gate64) + (cc.rec_rows.capacity() + cc.in_rows.capacity()) * 4 +
               (cc.rec_offs64.capacity() + cc.in_offs64.capacity()) * 8 + cc.level_start.capacity() * 8 + cc.level_range.capacity() * sizeof(LevelRange) + 4096;
    }

    void free_all() {
        void* ps[] = {d_seeds, d_keys, d_rkbytes, d_rk, d_rows, d_corr, d_wmask64, d_wcorr64, d_err, d_err0, d_dig, d_h, d_omit, d_offs, d_proof, d_pend_rec, d_pend_in, d_pend_pre,
                      d_wit_sum, proof_in_place ? nullptr : d_vproof, d_omit_v, d_omit64_v, d_hco, d_hco64, d_keep, d_keep64, d_onm, d_rk64, d_src};
        for (void* p : ps) ctx->release(p);
        for (auto& kv : kept) release_kept(kv.second);
        kept.clear();
        for (Transcript& t : tr) {
            ctx->release(t.d_tail);
            for (uint32_t* p : t.tree.node) ctx->release(p);
        }
    }
};

// n chaining values per proof into the proofs' trees (one proof for a single stream; cvs[b]: proof b's).  One level of the binary
// counter per loop trip: [pending?] ++ cur is paired up, an odd last node becomes the new pending.  The trees of a batch have the same
// shape (the same event counts), so every level is one k_b3_pairs_batched launch over them and one copy of their odd nodes; a single
// stream keeps launch_b3_pairs and a hipMemcpyAsync.
static int inc_absorb(rv_ctx* ctx, const std::vector<IncHash*>& Hs, const std::vector<uint32_t*>& cvs, uint64_t n, uint32_t R) {
    hipStream_t st = ctx->stream;
    const size_t B = Hs.size();
    for (IncHash* H : Hs)
        if (H->chunks != Hs[0]->chunks || H->full != Hs[0]->full || H->node.size() != Hs[0]->node.size()) {
            for (size_t b = 0; b < B; b++) {  // (cannot happen: the members see the same chunks)
                int rc = inc_absorb(ctx, {Hs[b]}, {cvs[b]}, n, R);
                if (rc) return rc;
            }
            return RV_OK;
        }
    std::vector<uint32_t*> cur(cvs);
    bool cur_owned = false;
    uint64_t n_cur = n;
    size_t lvl = 0;
    int rc;
    CopyBatch cp(st, B == 1);
    while (n_cur) {
        if (Hs[0]->node.size() <= lvl)
            for (IncHash* H : Hs) {
                uint32_t* p = nullptr;
                if ((rc = dalloc(ctx, (size_t)R * 8, &p))) return rc;
                H->node.push_back(p);
                H->full.push_back(0);
            }
        const bool pend = Hs[0]->full[lvl] != 0;
        const uint64_t total = n_cur + (pend ? 1 : 0), pairs = total / 2;
        std::vector<uint32_t*> out(B, nullptr);
        if (pairs) {
            uint32_t* blk = nullptr;  // (one allocation for the level's outputs of every proof)
            if ((rc = dalloc(ctx, (size_t)B * pairs * R * 8, &blk))) return rc;
            for (size_t b = 0; b < B; b++) out[b] = blk + b * pairs * R * 8;
            if (B == 1) launch_b3_pairs(st, pend ? Hs[0]->node[lvl] : nullptr, cur[0], pairs, R, out[0]);
            for (size_t b0 = 0; B > 1 && b0 < B; b0 += B3PairsBatch::MAX) {
                B3PairsBatch L{};
                for (size_t b = b0; b < std::min(B, b0 + B3PairsBatch::MAX); b++, L.n++) {
                    L.pending[L.n] = pend ? Hs[b]->node[lvl] : nullptr;
                    L.in[L.n] = cur[b];
                    L.out[L.n] = out[b];
                }
                launch_b3_pairs_batched(st, L, pairs, R);
            }
        }
        if (total & 1)
            for (size_t b = 0; b < B; b++) cp.add(Hs[b]->node[lvl], cur[b] + (size_t)(n_cur - 1) * R * 8, (size_t)R * 32);
        if ((rc = cp.finish("tree node copy"))) return rc;
        for (IncHash* H : Hs) H->full[lvl] = (total & 1) ? 1 : 0;
        if (cur_owned) ctx->release(cur[0]);  // (stream order keeps the arena's reuse behind the kernels that read it)
        cur = out;
        cur_owned = true;
        n_cur = pairs;
        lvl++;
    }
    if (cur_owned) ctx->release(cur[0]);
    for (IncHash* H : Hs) H->chunks += n;
    return RV_OK;
}

// the stream ends: its last chunk (chaining value in d_last, hashed with chunk counter H.chunks and the ROOT flag iff it
// is the only chunk) folded into the pending subtree roots
static void inc_finish(rv_ctx* ctx, const IncHash& H, const uint32_t* d_last, uint32_t R, uint32_t* d_digest) {
    B3FoldList L{};
    for (size_t l = 0; l < H.node.size() && L.n < 48; l++)
        if (H.full[l]) L.p[L.n++] = H.node[l];
    launch_b3_fold(ctx->stream, L, d_last, R, d_digest);
}

extern "C" void rv_stream_abort(rv_stream* S) {
    if (!S) return;
    (void)hipSetDevice(S->ctx->device);
    (void)hipStreamSynchronize(S->ctx->stream);
    for (rv_stream* m : S->bat) rv_stream_abort(m);
    S->bat.clear();
    S->free_all();
    delete S;
}

// seeds_on_device: `seeds` (not null) is 256 x 16 bytes in the memory of the context's device, written by work already queued on its stream
static int stream_begin_impl(rv_ctx* ctx, size_t z64_wires, size_t gf2_wires, const uint8_t* seeds, size_t max_chunk_ops, rv_stream** out,
                             bool seeds_on_device = false) {
    if (!ctx || !out) return RV_E_ARG;
    *out = nullptr;
    if (gf2_wires > 0x3FFFFFFFull || z64_wires > 0x3FFFFFFFull) return RV_E_UNSUPPORTED;
    HIPCHK(hipSetDevice(ctx->device));
    rv_stream* S = new rv_stream();
    S->ctx = ctx;
    S->z64_wires = z64_wires;
    S->gf2_wires = gf2_wires;
    S->compile_flags = ctx->compile_flags & RV_COMPILE_DEVICE_BITS;
    if (max_chunk_ops) S->max_chunk_ops = std::max<size_t>(max_chunk_ops, 1024);
    if (const char* e = getenv("RV_STREAM_KEEP_MB")) {
        S->keep_cap = (uint64_t)std::max(atoll(e), 0ll) << 20;
    } else {
        size_t free_b = 0, total_b = 0;
        if (hipMemGetInfo(&free_b, &total_b) != hipSuccess) (void)hipGetLastError(), total_b = free_b = 0;
        // (an eighth of the device, but never more than half of what is free NOW -- other contexts and streams share the device -- plus what this
        // context's arena holds idle and would hand back)
        S->keep_cap = std::min<uint64_t>({(uint64_t)total_b / 8, ((uint64_t)free_b + (uint64_t)ctx->cached_bytes) / 2, (uint64_t)32 << 30});
    }
    uint8_t drawn[RV_TOTAL_REPS * RV_KEY_SIZE];
    if (!seeds) {
        if (int rs = os_seeds(drawn, sizeof drawn)) {
            delete S;
            return rs;
        }
        seeds = drawn;
    }
    constexpr uint32_t R = rv_stream::R, NQ = rv_stream::NQ;
    int rc;
    auto fail = [&](int code) {
        rv_stream_abort(S);
        return code;
    };
    if ((rc = dalloc(ctx, (size_t)R * 16, &S->d_seeds)) || (rc = dalloc(ctx, (size_t)R * 128, &S->d_keys)) ||
        (rc = dalloc(ctx, (size_t)R * 8 * RK_BYTES, &S->d_rkbytes)) || (rc = dalloc(ctx, (size_t)RK_AREAS * 128 * NQ, &S->d_rk)) ||
        (rc = dalloc(ctx, 1, &S->d_err)) || (rc = dalloc(ctx, 1, &S->d_err0)) || (rc = dalloc(ctx, (size_t)TR_KINDS * R * 8, &S->d_dig)) ||
        (rc = dalloc(ctx, (size_t)R * 32, &S->d_h)) || (rc = dalloc(ctx, (size_t)8 * NQ, &S->d_pend_rec)) ||
        (rc = dalloc(ctx, (size_t)8 * NQ, &S->d_pend_in)) || (rc = dalloc(ctx, (size_t)8 * (NQ / 2), &S->d_pend_pre)))
        return fail(rc);
    for (int kind = 0; kind < TR_KINDS; kind++)
        if ((rc = dalloc(ctx, TR_KIND[kind].tail_bytes(), &S->tr[kind].d_tail))) return fail(rc);
    if (hipMemcpyAsync(S->d_seeds, seeds, (size_t)R * 16, seeds_on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, ctx->stream) != hipSuccess)
        return fail(RV_E_DEVICE);
    if (hipMemsetAsync(S->d_err, 0, sizeof(int), ctx->stream) != hipSuccess) return fail(RV_E_DEVICE);
    launch_expand_seeds(ctx->stream, S->d_seeds, R, S->d_keys);
    launch_key_schedule(ctx->stream, S->d_keys, R * 8, S->d_rkbytes);
    launch_bitslice_rk(ctx->stream, S->d_rkbytes, NQ, S->d_rk);
    if (hipStreamSynchronize(ctx->stream) != hipSuccess) return fail(RV_E_DEVICE);  // (`seeds` may live on this stack frame)
    *out = S;
    return RV_OK;
}

extern "C" int rv_stream_begin(rv_ctx* ctx, size_t z64_wires, size_t gf2_wires, const uint8_t* seeds, size_t max_chunk_ops, rv_stream** out) {
    return guarded([&] { return stream_begin_impl(ctx, z64_wires, gf2_wires, seeds, max_chunk_ops, out); });
}

extern "C" int rv_stream_set_compile_flags(rv_stream* S, uint32_t flags) {
    if (int rc = check_device_flags("rv_stream_set_compile_flags", flags)) return rc;
    if (!S || S->fed) return RV_E_ARG;
    S->compile_flags = flags;
    for (rv_stream* m : S->bat) m->compile_flags = flags;  // (a batch: the feed's host-side state is its first running member's)
    return RV_OK;
}

// wire store large enough for the chunk; the carried region survives a reallocation
static int stream_reserve(rv_stream* S, const Compiled& cc) {
    rv_ctx* ctx = S->ctx;
    constexpr uint32_t R = rv_stream::R, NQ = rv_stream::NQ;
    int rc;
    if (cc.n_rows > S->rows_cap) {
        const size_t cap = std::max<size_t>(cc.n_rows, S->rows_cap + S->rows_cap / 2);
        uint32_t* rows = nullptr;
        uint8_t* corr = nullptr;
        if ((rc = dalloc(ctx, cap * NQ, &rows)) || (rc = dalloc(ctx, cap * (NQ / 2), &corr))) return rc;
        if (S->d_rows) {
            HIPCHK(hipMemcpyAsync(rows, S->d_rows, S->gf2_wires * NQ * 4, hipMemcpyDeviceToDevice, ctx->stream));
            HIPCHK(hipMemcpyAsync(corr, S->d_corr, S->gf2_wires * (NQ / 2), hipMemcpyDeviceToDevice, ctx->stream));
        } else {  // every wire starts as the constant zero (interpreter/single.rs:16)
            HIPCHK(hipMemsetAsync(rows, 0, std::max<size_t>(S->gf2_wires, 1) * NQ * 4, ctx->stream));
            HIPCHK(hipMemsetAsync(corr, 0, std::max<size_t>(S->gf2_wires, 1) * (NQ / 2), ctx->stream));
        }
        ctx->release(S->d_rows);
        ctx->release(S->d_corr);
        S->d_rows = rows;
        S->d_corr = corr;
        S->rows_cap = cap;
    }
    if (cc.n_ssa64 > S->ssa64_cap) {
        const size_t cap = std::max<size_t>(cc.n_ssa64, S->ssa64_cap + S->ssa64_cap / 2);
        uint64_t *wm = nullptr, *wc = nullptr;
        if ((rc = dalloc(ctx, cap * R * 8, &wm)) || (rc = dalloc(ctx, cap * R, &wc))) return rc;
        const size_t keep = 1 + S->z64_wires;  // slot 0 = the zero wire, then one slot per wire index
        if (S->d_wmask64) {
            HIPCHK(hipMemcpyAsync(wm, S->d_wmask64, keep * R * 64, hipMemcpyDeviceToDevice, ctx->stream));
            HIPCHK(hipMemcpyAsync(wc, S->d_wcorr64, keep * R * 8, hipMemcpyDeviceToDevice, ctx->stream));
        } else {
            HIPCHK(hipMemsetAsync(wm, 0, keep * R * 64, ctx->stream));
            HIPCHK(hipMemsetAsync(wc, 0, keep * R * 8, ctx->stream));
        }
        ctx->release(S->d_wmask64);
        ctx->release(S->d_wcorr64);
        S->d_wmask64 = wm;
        S->d_wcorr64 = wc;
        S->ssa64_cap = cap;
    }
    return RV_OK;
}

// 64-bit digest of the op stream (pass 2 must see pass 1's ops): a sum of per-op mixes keyed by the op's position, so it
// does not depend on how the stream was cut and the pieces of a feed can be digested on the threads that compile them
static uint64_t ops_digest(const rv_op* ops, size_t n, uint64_t first_index) {
    uint64_t sum = 0;
    for (size_t i = 0; i < n; i++) {
        const rv_op& o = ops[i];
        uint64_t h = (first_index + i) * 0x9E3779B97F4A7C15ull;
        const uint64_t w[3] = {(uint64_t)o.domain | (uint64_t)o.opcode << 8 | (uint64_t)o.dst << 32, (uint64_t)o.a | (uint64_t)o.b << 32, o.imm};
        for (uint64_t x : w) {
            h ^= x + 0x9E3779B97F4A7C15ull + (h << 6) + (h >> 2);
            h *= 0xFF51AFD7ED558CCDull;
            h ^= h >> 29;
        }
        sum += h;
    }
    return sum;
}

// the same for the witness elements a chunk consumes (GF(2) bytes, then Z64 words), keyed by their input ordinals
static uint64_t wit_digest(const uint8_t* w2, size_t n2, uint64_t first2, const uint64_t* w64, size_t n64, uint64_t first64) {
    uint64_t sum = 0;
    auto mix = [](uint64_t pos, uint64_t x) {
        uint64_t h = pos * 0x9E3779B97F4A7C15ull;
        h ^= x + 0x9E3779B97F4A7C15ull + (h << 6) + (h >> 2);
        h *= 0xFF51AFD7ED558CCDull;
        return h ^ (h >> 29);
    };
    for (size_t i = 0; i < n2; i++) sum += mix(2 * (first2 + i), w2[i] & 1u);
    for (size_t i = 0; i < n64; i++) sum += mix(2 * (first64 + i) + 1, w64[i]);
    return sum;
}

// one piece compiled as a streaming chunk.  at: the transcript offsets to compile it at (null: zero -- relocate_chunk moves it later)
static int stream_compile_piece(const rv_stream* S, const rv_op* ops, size_t n_ops, uint32_t mask_phase, uint32_t mask64_phase, rv_circuit** out,
                                const ChunkStart* at = nullptr) {
    ChunkStart cs;
    if (at) cs = *at;
    cs.mask_phase = mask_phase;
    cs.mask64_phase = mask64_phase;
    rv_circuit* c = new rv_circuit();
    c->ctx = S->ctx;
    const int rc = compile_ops(ops, n_ops, S->z64_wires, S->gf2_wires, c->cc, &cs);
    if (rc) {
        delete c;
        return rc;
    }
    *out = c;
    return RV_OK;
}

// the error flags of the proofs' chunks since the pass began, read with one wait.  The prover: the first witness whose AssertZero
// failed is named in rv_last_error (RV_E_WITNESS_INVALID); the verifier: RV_DEV_ZERO_CHECK goes into each proof's dev_flags.
static int stream_read_errs(const std::vector<rv_stream*>& proofs, const char* what) {
    hipStream_t st = proofs[0]->ctx->stream;
    std::vector<int> err(proofs.size(), 0);
    for (size_t b = 0; b < proofs.size(); b++)
        if (hipMemcpyAsync(&err[b], proofs[b]->d_err, sizeof(int), hipMemcpyDeviceToHost, st) != hipSuccess)
            return hip_fail(hipGetLastError(), what, __FILE__, __LINE__);
    if (hipStreamSynchronize(st) != hipSuccess) return hip_fail(hipGetLastError(), what, __FILE__, __LINE__);
    for (size_t b = 0; b < proofs.size(); b++) {
        if (proofs[b]->pass == 3) {
            proofs[b]->dev_flags |= err[b];  // RV_DEV_ZERO_CHECK: an AssertZero of an opened repetition (the strict verifier reads it at the end)
        } else if (err[b]) {
            char buf[96];
            snprintf(buf, sizeof buf, "an AssertZero fails for witness %zu of the stream", b);
            g_last_error = buf;
            return RV_E_WITNESS_INVALID;
        }
    }
    return RV_OK;
}

// the witnesses of a feed: proof b's elements at gf2 + b * stride2 and z64 + b * stride64, n_gf2 / n_z64 of them still unconsumed
struct WitnessRows {
    const uint8_t* gf2;
    size_t n_gf2, stride2;
    const uint64_t* z64;
    size_t n_z64, stride64;
    bool dev = false;  // the rows are in the memory of the stream's device (rv_stream_feed_wdev)
    const uint8_t* gf2_of(size_t b) const { return gf2 ? gf2 + b * stride2 : nullptr; }
    const uint64_t* z64_of(size_t b) const { return z64 ? z64 + b * stride64 : nullptr; }
    void advance(size_t u2, size_t u64) {
        gf2 = gf2 ? gf2 + u2 : gf2;
        n_gf2 -= u2;
        z64 = z64 ? z64 + u64 : z64;
        n_z64 -= u64;
    }
};

// One chunk of the gate stream through masks -> interpreter -> (pass 1, verifier) chunk hashes / (pass 2) openings, as a sequence of
// steps that run() calls in order:
//   plan (offsets, relocate, witness / CTR-range checks, kept-chunk match) -> upload -> per proof: buffers (kept / keep / scratch),
//   carried events in, witness copy, verifier's supplied values, masks, parameter block, k_shard_init, (single) level loop ->
//   (batch) parameter upload + batched level loop -> hashing: chunk hashes, trees, tails -> pass 2: openings per proof ->
//   kept-set consistency -> error flags / no-wait -> counters.
// The compile, relocation and gate upload happen once; a batch (proofs.size() > 1) takes each step for all its proofs together where
// it can: the small copies go into one k_copy_rows_batched launch per step (CopyBatch), the level loop is launch_levels_batched over
// per-proof parameter blocks (the proof in gridDim.y, as rv_prove_batch), the trees grow through k_b3_pairs_batched; the masks, chunk
// hashes and openings go proof after proof, with no wait between them.  A single stream keeps its own launches.
// The host side of a chunk: levelising 10^6 ops takes ~0.1 s on one core, ~200 times the chunk's GPU work, and needs nothing of the
// stream's state but the two ShareGen phases (transcript offsets are added afterwards, relocate_chunk).  A feed of several chunks
// therefore compiles them on worker threads ahead of the GPU (stream_feed_impl).
// where the next chunk of the stream starts: the ShareGen phases and the carried events in front of its own (pass 1 and the verifier:
// the unhashed tails; pass 2: the items short of a byte)
static ChunkStart stream_chunk_start(const rv_stream* S) {
    ChunkStart cs;
    cs.mask_phase = (uint32_t)(S->run.masks % 128);
    cs.mask64_phase = (uint32_t)(S->run.masks64 % 2);
    if (S->pass != 2)
        set_carried(cs, S->tr[TR_PRE].tail, S->tr[TR_ON].tail, S->tr[TR_PRE64].tail, S->tr[TR_ON64].tail);
    else
        set_carried(cs, S->pend_pre, S->pend_rec + S->pend_in, 0, 0);
    return cs;
}

struct ChunkRun {
    static constexpr uint32_t R = rv_stream::R, NQ = rv_stream::NQ;
    using Clock = std::chrono::steady_clock;
    struct ProofBufs {  // one proof's buffers of the chunk
        uint8_t* tr[TR_KINDS] = {nullptr, nullptr, nullptr, nullptr};  // its transcripts, carried events in front
        uint64_t pitch[TR_KINDS] = {0, 0, 1, 1};                      // words per repetition of the Z64 ones
        rv_stream::Kept* kp = nullptr;                                // pass 1's kept transcripts of this chunk (use_kept)
        uint8_t* d_wit = nullptr;
        uint64_t *d_wit64 = nullptr, *d_masks64 = nullptr;
        uint32_t *d_sup_in = nullptr, *d_sup_corr = nullptr, *d_sup_rec = nullptr;  // verifier: the values the proof supplies
        uint64_t *d_sup_in64 = nullptr, *d_sup_corr64 = nullptr, *d_sup_rec64 = nullptr;
        uint32_t* on() const { return (uint32_t*)tr[TR_ON]; }
        uint8_t* pre() const { return tr[TR_PRE]; }
        uint64_t* on64() const { return (uint64_t*)tr[TR_ON64]; }
        uint64_t* pre64() const { return (uint64_t*)tr[TR_PRE64]; }
    };

    rv_stream* const S;                      // proofs[0]: holds the host-side state (cache, counts, pass)
    const std::vector<rv_stream*>& proofs;   // the proofs the chunk runs for
    rv_circuit* c;                           // the chunk, compiled with the phases the stream is at now (consumed here)
    const uint64_t digest;                   // ops_digest of the chunk's ops at their position in the stream
    const size_t n_ops;
    const WitnessRows wit;
    rv_ctx* const ctx;
    const hipStream_t st;
    const bool p1, ver, hashing, batched;    // ver: the streaming verifier ("pass 3"): verify-mode chunks, transcripts hashed as in pass 1
    const Compiled& cc;
    const uint64_t first_op;
    const bool has64;
    const uint64_t first_block, n_blocks, first_block64, n_blocks64;  // the chunk's CTR blocks of the two mask generators
    ChunkStart cs;                           // where the chunk starts: mask phases, carried events
    bool use_kept = false;                   // pass 2 of a chunk whose transcripts pass 1 kept: only the openings are taken from them
    bool no_wait = false;
    bool tr64 = false;                       // the chunk has Z64 transcripts
    uint64_t on_rows = 1, pre_rows = 1;      // rows of its GF(2) transcript buffers
    size_t used_gf2 = 0, used_z64 = 0;       // witness elements a chunk that ran has consumed, per proof
    std::vector<void*> tmp;                  // scratch, released when the chunk is issued (the next chunk's buffers reuse it behind it on the stream)
    std::vector<ProofBufs> pbs;
    std::vector<InterpParams> pps;
    std::vector<Interp64Params> pp64s;
    CopyBatch cp;
    Clock::time_point t_begin = Clock::now(), t_reloc, t_up, t_alloc, t_issue, t_gpu;

    ChunkRun(const std::vector<rv_stream*>& proofs_, rv_circuit* c_, uint64_t digest_, size_t n_ops_, const WitnessRows& wit_)
        : S(proofs_[0]), proofs(proofs_), c(c_), digest(digest_), n_ops(n_ops_), wit(wit_), ctx(S->ctx), st(ctx->stream), p1(S->pass == 1), ver(S->pass == 3),
          hashing(p1 || ver), batched(proofs_.size() > 1), cc(c_->cc), first_op(S->run.n_ops), has64(!cc.gates64.empty()),
          first_block(S->run.masks / 128), n_blocks(cc.n_masks_pad / 128), first_block64(S->run.masks64 / 2), n_blocks64((cc.n_masks64 + 1) / 2),
          cs(stream_chunk_start(S)), pbs(proofs_.size()), pps(proofs_.size()), pp64s(proofs_.size()), cp(st, !batched) {}

    // carried: the transcript offsets c's arrays already hold (zero for a fresh compile, pass 1's for a chunk out of the cache)
    int run(const ChunkStart& carried) {
        if (int rc = plan(carried)) {  // (nothing of the chunk is on the stream yet)
            rv_circuit_destroy(c);
            return rc;
        }
        return finish(issue());
    }

    int plan(const ChunkStart& carried) {
        static const bool stats = getenv("RV_STREAM_STATS") != nullptr;
        if (!same_carried(cs, carried)) {
            static int moved = 0;
            if (stats && ++moved <= 3) fprintf(stderr, "[rv stream] a chunk's transcript offsets are moved on the main thread (not predicted, or a single-piece feed)\n");
            c->staged = nullptr;  // (a worker's page-locked copy of the arrays predates this move)
        }
        relocate_to(c->cc, carried, cs);
        t_reloc = Clock::now();
        on_rows = std::max<uint64_t>(cc.n_on, 1), pre_rows = std::max<uint64_t>(cc.n_pre, 1);  // (the compiled counters include the carried events)
        tr64 = has64 || cc.on_words64 || cc.pre_words64;
        if (!ver && (cc.n_in > wit.n_gf2 || cc.n_in64 > wit.n_z64)) return RV_E_WITNESS_SHORT;
        if (!ver && ((cc.n_in && !wit.gf2) || (cc.n_in64 && !wit.z64))) return RV_E_ARG;
        // the mask kernels' first-round shortcut covers CTR indices below 2^24 (internal.h)
        if (first_block + n_blocks > RV_MAX_CTR_BLOCKS || first_block64 + n_blocks64 > RV_MAX_CTR_BLOCKS) return RV_E_UNSUPPORTED;
        // pass 2 of a chunk whose transcripts pass 1 kept: for every proof of the stream or for none
        if (S->pass == 2) {
            size_t n_match = 0, n_found = 0;
            for (rv_stream* Q : proofs) {
                auto it = Q->kept.find(first_op);
                if (it == Q->kept.end()) continue;
                n_found++;
                n_match += it->second.n_ops == n_ops && it->second.digest == digest;
            }
            use_kept = n_found && n_match == proofs.size();
            if (n_found && !use_kept) drop_kept_chunk();  // (cut differently, or other ops: finish reports those) -- of no use any more
        }
        if (use_kept)
            for (rv_stream* Q : proofs) Q->p2_skipped = true;
        if (!use_kept && S->pass == 2 && S->p2_skipped) {
            g_last_error = "rv_stream_same_cuts was promised, but pass 2 is not fed in pass 1's pieces";
            return RV_E_ARG;
        }
        return RV_OK;
    }

    // every step from the upload on; whatever it returns goes through finish()
    int issue() {
        int rc;
        if ((rc = upload())) return rc;
        for (size_t bi = 0; bi < proofs.size(); bi++)
            if ((rc = issue_proof(bi))) return rc;
        if ((rc = cp.finish("carried events"))) return rc;  // (the carried events are in place before any level runs)
        if (batched && !use_kept && (rc = run_levels_batched())) return rc;
        if (hashing && (rc = hash_transcripts())) return rc;
        for (size_t bi = 0; bi < proofs.size() && !hashing; bi++)
            if ((rc = open_proof(bi))) return rc;
        if ((rc = cp.finish("pending rows"))) return rc;
        keep_for_all_or_none();
        if (!ver && wit.dev && (rc = digest_witness_on_device())) return rc;  // (in front of the chunk's or the feed's wait: the last read of the caller's rows)
        t_issue = Clock::now();
        if ((rc = settle())) return rc;
        count();
        return RV_OK;
    }

    // With no wait per chunk, work of this chunk may still be in flight: an error waits for the stream before the chunk, its scratch
    // and a matched Kept entry go back.  A successful pass-1 chunk goes into the compiled-chunk cache.
    int finish(int code) {
        if (code != RV_OK) (void)hipStreamSynchronize(st);
        for (void* p : tmp) ctx->release(p);
        tmp.clear();
        if (use_kept) drop_kept_chunk();  // (back to the arena: whatever takes them next is ordered behind this chunk's kernels on the stream)
        if (code == RV_OK && p1) {        // keep the compiled chunk for pass 2 (host arrays only; the device copies go back to the arena)
            static const uint64_t cap = (uint64_t)(getenv("RV_STREAM_CACHE_MB") ? std::max(atoi(getenv("RV_STREAM_CACHE_MB")), 0) : 1024) << 20;
            const uint64_t b = rv_stream::compiled_bytes(c->cc);
            if (S->cache_bytes + b <= cap) {
                rv_stream::CachedPiece& k = S->cache[first_op];
                k.n_ops = n_ops;
                k.digest = digest;
                k.at = cs;
                k.cc = std::move(c->cc);
                S->cache_bytes += b;
            }
        }
        rv_circuit_destroy(c);
        c = nullptr;
        return code;
    }

    void drop_kept_chunk() {
        for (rv_stream* Q : proofs) {
            auto it = Q->kept.find(first_op);
            if (it == Q->kept.end()) continue;
            Q->release_kept(it->second);
            Q->kept.erase(it);
        }
    }
    void drop_all_kept() {
        for (rv_stream* Q : proofs) {
            for (auto& kv : Q->kept) Q->release_kept(kv.second);
            Q->kept.clear();
            Q->keep_cap = 0;
        }
    }
    // device scratch of the chunk
    template <class T>
    int take(size_t bytes, T** out) {
        void* p = nullptr;
        int r = ctx->alloc(bytes, &p);
        bool any_kept = false;
        for (rv_stream* Q : proofs) any_kept = any_kept || !Q->kept.empty();
        if (r == RV_E_NOMEM && !use_kept && any_kept) {  // the kept transcripts are a convenience of pass 2: they go before a chunk fails for memory
            (void)hipStreamSynchronize(st);
            drop_all_kept();
            ctx->trim();
            r = ctx->alloc(bytes, &p);
        }
        if (!r) tmp.push_back(p);
        *out = (T*)p;
        return r;
    }
    int hip_code(hipError_t e, const char* what) { return e == hipSuccess ? RV_OK : hip_fail(e, what, __FILE__, __LINE__); }

    // no wait per chunk (the feed ends with one: stream_feed_settle) unless the phase timers are on or the piece is not in a ring slot
    int upload() {
        if (!use_kept) {
            if (int rc = circuit_upload(ctx, c, !ctx->profiling)) {
                c = nullptr;  // (circuit_upload destroys the circuit on every failure)
                return rc;
            }
        }
        no_wait = !use_kept && c->upload_pending && !(ver && has64);  // (the verifier's Z64 chunks feed a copy from a local array)
        t_up = t_alloc = Clock::now();
        return RV_OK;
    }

    // the proof's transcript buffers: pass 1's kept ones, new ones to keep for pass 2, or scratch; then the rest of its scratch
    int proof_buffers(rv_stream* P, ProofBufs& q) {
        int rc;
        uint64_t &onw = q.pitch[TR_ON64], &prew = q.pitch[TR_PRE64];
        onw = std::max<uint64_t>(cc.on_words64, 1), prew = std::max<uint64_t>(cc.pre_words64, 1);
        if (use_kept) {
            rv_stream::Kept* kp = q.kp = &P->kept[first_op];
            // the chunk's own events sit behind kp->on0 carried ones in the kept buffers and belong behind cs.on0 now
            q.tr[TR_ON] = (uint8_t*)(kp->d_on + ((int64_t)kp->on0 - (int64_t)cs.on0) * (int64_t)NQ);
            q.tr[TR_PRE] = kp->d_pre + ((int64_t)kp->pre0 - (int64_t)cs.pre0) * (int64_t)(NQ / 2);
            if (tr64) {
                if (!kp->d_on64 || !kp->d_pre64) return RV_E_DEVICE;
                q.tr[TR_ON64] = (uint8_t*)(kp->d_on64 + kp->on64_0);  // (pass 2 carries no Z64 words: cs.on_words64_0 = 0)
                q.tr[TR_PRE64] = (uint8_t*)(kp->d_pre64 + kp->pre64_0);
                onw = kp->onw;
                prew = kp->prew;
            }
            return RV_OK;
        }
        // pass 1 keeps the transcripts for pass 2 while they fit the budget
        constexpr uint64_t HEAD_ON = 16, HEAD_PRE = 8;
        const uint64_t keep_need = (on_rows + HEAD_ON) * NQ * 4 + (pre_rows + HEAD_PRE) * (NQ / 2) + (tr64 ? (onw + prew) * R * 8 : 0);
        // (the kept chunks stay a suffix of the stream: the oldest ones make room; a chunk that cannot be kept empties the set)
        const bool keep = p1 && S->same_cuts && keep_need <= P->keep_cap;
        if (p1 && S->same_cuts)
            while (!P->kept.empty() && (!keep || P->kept_bytes + keep_need > P->keep_cap)) {
                P->release_kept(P->kept.begin()->second);
                P->kept.erase(P->kept.begin());
            }
        if (keep) {
            rv_stream::Kept k;
            k.n_ops = n_ops, k.digest = digest, k.bytes = keep_need;
            k.on0 = cs.on0, k.pre0 = cs.pre0, k.on64_0 = cs.on_words64_0, k.pre64_0 = cs.pre_words64_0, k.onw = onw, k.prew = prew;
            int r = ctx->alloc((on_rows + HEAD_ON) * NQ * 4, &k.on_base);
            if (!r) r = ctx->alloc((pre_rows + HEAD_PRE) * (NQ / 2), &k.pre_base);
            if (!r && tr64) r = ctx->alloc(onw * R * 8, (void**)&k.d_on64);
            if (!r && tr64) r = ctx->alloc(prew * R * 8, (void**)&k.d_pre64);
            if (r) {  // (no room after all: nothing is kept from here back -- the kept chunks must be a suffix -- and the chunk runs as ever)
                ctx->release(k.on_base), ctx->release(k.pre_base), ctx->release(k.d_on64), ctx->release(k.d_pre64);
                for (auto& kv : P->kept) P->release_kept(kv.second);
                P->kept.clear();
                P->keep_cap = 0;
            } else {
                k.d_on = (uint32_t*)k.on_base + HEAD_ON * NQ;
                k.d_pre = (uint8_t*)k.pre_base + HEAD_PRE * (NQ / 2);
                q.tr[TR_ON] = (uint8_t*)k.d_on, q.tr[TR_PRE] = k.d_pre, q.tr[TR_ON64] = (uint8_t*)k.d_on64, q.tr[TR_PRE64] = (uint8_t*)k.d_pre64;
                P->kept_bytes += keep_need;
                P->kept_peak = std::max(P->kept_peak, P->kept_bytes);
                P->kept[first_op] = k;
            }
        }
        if (!q.tr[TR_ON]) {
            if ((rc = take(on_rows * NQ * 4, &q.tr[TR_ON])) || (rc = take(pre_rows * (NQ / 2), &q.tr[TR_PRE]))) return rc;
            if (tr64 && ((rc = take(onw * R * 8, &q.tr[TR_ON64])) || (rc = take(prew * R * 8, &q.tr[TR_PRE64])))) return rc;
        }
        if ((rc = take(std::max<size_t>(cc.n_in, 1), &q.d_wit))) return rc;
        if (tr64 && ((rc = take(std::max<size_t>(cc.n_in64, 1) * 8, &q.d_wit64)) || (rc = take(std::max<uint64_t>(n_blocks64, 1) * 2 * R * 64, &q.d_masks64)))) return rc;
        return RV_OK;
    }

    // carried events in front of the chunk's own: the unhashed tails (pass 1, verifier) or the pending rows (pass 2)
    void carry_in(rv_stream* P, const ProofBufs& q) {
        if (hashing) {
            for (int kind : {TR_ON, TR_PRE, TR_ON64, TR_PRE64})
                if (q.tr[kind]) TR_KIND[kind].copy(cp, q.tr[kind], q.pitch[kind], P->tr[kind].d_tail, TR_KIND[kind].unit, P->tr[kind].tail);
        } else {
            CopySegs segs{};
            if (P->pend_rec) segs.add(P->d_pend_rec, q.on(), P->pend_rec * NQ * 4);
            if (P->pend_in) segs.add(P->d_pend_in, q.on() + (size_t)P->pend_rec * NQ, P->pend_in * NQ * 4);
            if (P->pend_pre) segs.add(P->d_pend_pre, q.pre(), P->pend_pre * (NQ / 2));
            cp.add(segs);
        }
    }

    // verifier: the values the proof supplies for this chunk's items (verifier/online.rs:122-183), rebuilt from the vectors' items
    // [items so far, + this chunk's) -- at any bit offset
    int supplied_values(rv_stream* P, ProofBufs& q) {
        int rc;
        const uint32_t SNQ = P->sup_nq;
        if ((rc = take(std::max<uint64_t>(cc.n_in, 1) * SNQ * 4, &q.d_sup_in)) || (rc = take(std::max<uint64_t>(cc.n_pre, 1) * SNQ * 4, &q.d_sup_corr)) ||
            (rc = take(std::max<uint64_t>(cc.n_rec, 1) * SNQ * 4, &q.d_sup_rec)))
            return rc;
        // (corrections are addressed by their transcript row: the chunk's own start behind the cs.pre0 carried rows)
        launch_unpack_bits(st, P->d_vproof, P->d_src + 4 * R, P->d_src + 5 * R, P->d_omit_v, cc.n_in, NQ, 1, q.d_sup_in, SNQ, P->run.n_in);
        launch_unpack_bits(st, P->d_vproof, P->d_src + 2 * R, P->d_src + 3 * R, P->d_omit_v, cc.n_pre - cs.pre0, NQ, 1, q.d_sup_corr + (size_t)cs.pre0 * SNQ, SNQ,
                           P->run.n_pre);
        launch_unpack_bits(st, P->d_vproof, P->d_src + 0 * R, P->d_src + 1 * R, P->d_omit_v, cc.n_rec, NQ, 0, q.d_sup_rec, SNQ, P->run.n_rec);
        if (!has64) return RV_OK;
        uint64_t* d_src64 = nullptr;
        const uint32_t SR = P->sup_r;
        if ((rc = take((size_t)6 * R * 8, &d_src64)) || (rc = take(std::max<uint64_t>(cc.n_in64, 1) * SR * 8, &q.d_sup_in64)) ||
            (rc = take(std::max<uint64_t>(cc.n_corr64, 1) * SR * 8, &q.d_sup_corr64)) || (rc = take(std::max<uint64_t>(cc.n_rec64, 1) * SR * 8, &q.d_sup_rec64)))
            return rc;
        // 8-byte items: the chunk's first item is a byte offset into every vector
        std::vector<uint64_t>& src64c = P->src64c;  // (feeds an asynchronous copy: the chunk's final synchronisation comes before it is written again)
        src64c = P->src64;
        const uint64_t first[3] = {P->run.n_rec64, P->run.n_corr64, P->run.n_in64};
        for (int v = 0; v < 3; v++)
            for (uint32_t r = 0; r < R; r++) {
                uint64_t &off = src64c[(size_t)(2 * v) * R + r], &len = src64c[(size_t)(2 * v + 1) * R + r];
                const uint64_t skip = std::min(len, 8 * first[v]);
                off += skip;
                len -= skip;
            }
        if ((rc = hip_code(hipMemcpyAsync(d_src64, src64c.data(), src64c.size() * 8, hipMemcpyHostToDevice, st), "supplied Z64 offsets"))) return rc;
        launch_unpack_supplied64(st, cc, P->d_vproof, d_src64, P->d_omit64_v, R, q.d_sup_in64, q.d_sup_corr64, q.d_sup_rec64, SR);
        return RV_OK;
    }

    void fill_params(rv_stream* P, const ProofBufs& q, InterpParams& p, Interp64Params& p64) {
        p.NQ = NQ;
        p.rows = P->d_rows;
        p.corr = P->d_corr;
        p.on = q.on();
        p.pre = q.pre();
        p.wit = q.d_wit;
        p.err = P->d_err;
        p64.R = R;
        p64.wmask = P->d_wmask64;
        p64.wcorr = P->d_wcorr64;
        p64.masks = q.d_masks64;
        p64.on = q.on64();
        p64.pre = q.pre64();
        p64.on_words = q.pitch[TR_ON64];
        p64.pre_words = q.pitch[TR_PRE64];
        p64.wit = q.d_wit64;
        p64.corr2 = P->d_corr;
        p64.masks2 = P->d_rows;
        p64.NQ = NQ;
        p64.err = P->d_err;
        if (ver) {
            p.on_mask = P->d_onm;
            p.sup_in = q.d_sup_in;
            p.sup_corr = q.d_sup_corr;
            p.sup_rec = q.d_sup_rec;
            p.sup_nq = P->sup_nq;
            p64.omit = P->d_omit64_v;
            p64.sup_in = q.d_sup_in64;
            p64.sup_corr = q.d_sup_corr64;
            p64.sup_rec = q.d_sup_rec64;
            p64.sup_r = P->sup_r;
        }
    }

    // one proof's share of the chunk up to its levels (a batch runs the levels of all proofs afterwards)
    int issue_proof(size_t bi) {
        rv_stream* P = proofs[bi];
        ProofBufs& q = pbs[bi];
        int rc;
        if ((rc = stream_reserve(P, cc)) || (rc = proof_buffers(P, q))) return rc;
        const uint64_t ws = cc.n_rows * (uint64_t)(NQ * 4 + NQ / 2) + on_rows * NQ * 4 + pre_rows * (NQ / 2) + cc.gates.size() * sizeof(Gate) +
                            (has64 ? (q.pitch[TR_ON64] + q.pitch[TR_PRE64]) * R * 8 + n_blocks64 * 2 * R * 64 + cc.n_ssa64 * (uint64_t)R * 72 : 0);
        P->peak_bytes = std::max(P->peak_bytes, ws);
        carry_in(P, q);
        if (!ver && !q.kp) {
            // (device rows: device-to-device; a batch's Z64 words -- 8-byte aligned -- ride in the step's small-copy launch, the GF(2)
            // bytes have alignment 1 and keep the copy call)
            const hipMemcpyKind kind = wit.dev ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice;
            if (cc.n_in && (rc = hip_code(hipMemcpyAsync(q.d_wit, wit.gf2_of(bi), cc.n_in, kind, st), "GF(2) witness"))) return rc;
            if (cc.n_in64 && wit.dev && batched)
                cp.add(q.d_wit64, wit.z64_of(bi), cc.n_in64 * 8);
            else if (cc.n_in64 && (rc = hip_code(hipMemcpyAsync(q.d_wit64, wit.z64_of(bi), cc.n_in64 * 8, kind, st), "Z64 witness")))
                return rc;
            stream_traffic(wit.dev ? 1 : 0, cc.n_in + cc.n_in64 * 8);
        }
        if (ver && (rc = supplied_values(P, q))) return rc;
        if (bi == 0) t_alloc = Clock::now();
        // masks of this chunk: CTR blocks [first_block, first_block + n_blocks) (the first one may be shared with the previous chunk: its
        // leading masks were consumed there and are simply regenerated).  (verifier: the omitted player of every opened repetition is
        // skipped, generator/batch.rs:32-34; the Z64 transcript of a repetition has its own keys, online.rs:101-113)
        ctx->phase(RV_PH_MASKS);
        if (!q.kp) {
            launch_aes_gf2_masks(st, P->d_rk, ver ? P->d_keep : nullptr, NQ, first_block, n_blocks, P->d_rows + (size_t)cc.row_prg_base * NQ);
            if (n_blocks64 && q.d_masks64)
                launch_aes_z64_masks(st, ver ? P->d_rk64 : P->d_rk, ver ? P->d_keep64 : nullptr, NQ, n_blocks64, q.d_masks64, first_block64);
            ctx->count(2);
        }
        ctx->phase(-1);
        fill_params(P, q, pps[bi], pp64s[bi]);
        if (q.kp) return RV_OK;
        launch_shard_init(st, P->d_err0, P->d_rows + (size_t)cc.zero_row * NQ, NQ, P->d_corr + (size_t)cc.zero_row * (NQ / 2), NQ / 2);
        if (batched) return RV_OK;
        rv_shard sh;  // the level loop only needs the circuit and the context
        sh.ctx = ctx;
        sh.c = c;
        sh.R = R;
        sh.NQ = NQ;
        rc = shard_run_levels(&sh, ver ? MODE_VERIFY : MODE_PROVE, pps[bi], pp64s[bi]);
        ctx->phase(-1);
        return rc;
    }

    // a batch: the proofs' parameter blocks go to the device in one copy out of a page-locked slot, then one level loop over them
    int run_levels_batched() {
        const size_t NB = proofs.size();
        const size_t o64 = (NB * sizeof(InterpParams) + 63) & ~(size_t)63, bytes = o64 + NB * sizeof(Interp64Params);
        int slot = 0, rc;
        uint8_t* hp = ctx->open_slot(bytes, &slot);
        if (!hp) return RV_E_NOMEM;
        memcpy(hp, pps.data(), NB * sizeof(InterpParams));
        memcpy(hp + o64, pp64s.data(), NB * sizeof(Interp64Params));
        uint8_t* dp = nullptr;
        if ((rc = take(bytes, &dp))) return rc;
        if ((rc = hip_code(hipMemcpyAsync(dp, hp, bytes, hipMemcpyHostToDevice, st), "parameter blocks")) ||
            (rc = hip_code(hipEventRecord(ctx->ev_open[slot], st), "parameter blocks")))
            return rc;
        ctx->phase(RV_PH_INTERP);
        launch_levels_batched(ctx, c, ver ? MODE_VERIFY : MODE_PROVE, (const InterpParams*)dp, has64 ? (const Interp64Params*)(dp + o64) : nullptr, NB);
        ctx->phase(-1);
        return hipGetLastError() != hipSuccess ? RV_E_DEVICE : RV_OK;
    }

    // chunk chaining values of everything but the stream's last (possibly incomplete) chunk, into the trees: per kind of transcript
    // the chunk hashes of every proof, then their trees (together when batched), then their tails
    int hash_transcripts() {
        int rc;
        ctx->phase(RV_PH_HASH);
        const uint64_t totals[TR_KINDS] = {cc.n_pre, cc.n_on, cc.pre_words64, cc.on_words64};
        for (int kind = 0; kind < TR_KINDS; kind++) {
            const TranscriptKind& K = TR_KIND[kind];
            const uint64_t tail = K.tail_of(totals[kind]), hashed = totals[kind] - tail, n_chunks = hashed / K.unit;
            std::vector<IncHash*> Hs;
            std::vector<uint32_t*> cvsv;
            for (size_t bi = 0; bi < proofs.size(); bi++) {
                rv_stream::Transcript& T = proofs[bi]->tr[kind];
                const ProofBufs& q = pbs[bi];
                if (n_chunks) {
                    uint32_t* cvs = nullptr;
                    if ((rc = take((size_t)n_chunks * R * 32, &cvs))) return rc;
                    K.hash(st, q.tr[kind], q.pitch[kind], hashed, cvs, T.tree.chunks, 0);
                    Hs.push_back(&T.tree);
                    cvsv.push_back(cvs);
                }
                K.copy(cp, T.d_tail, K.unit, q.tr[kind] + hashed * K.ev_bytes, q.pitch[kind], tail);
                T.tail = tail;
            }
            if (n_chunks && (rc = inc_absorb(ctx, Hs, cvsv, n_chunks, R))) return rc;
        }
        rc = cp.finish("transcript tails");
        ctx->phase(-1);
        return rc;
    }

    // pass 2: openings of the challenged repetitions for this chunk's items.  Eight items make a byte, so a vector's last (< 8) items
    // wait in d_pend_* for the next chunk; what is extracted is always whole bytes.
    int open_proof(size_t bi) {
        rv_stream* P = proofs[bi];
        const ProofBufs& q = pbs[bi];
        int rc;
        ctx->phase(RV_PH_OPEN);
        // the chunk's host-built tables in one page-locked blob: [dst 6R u64 | OnlineList | rec_offs64 | in_offs64 | rec_list | in_list]
        const size_t n_recl = (size_t)P->pend_rec + cc.rec_rows.size(), n_inl = (size_t)P->pend_in + cc.in_rows.size();
        const size_t o_dst = 0, o_ol = o_dst + (size_t)6 * R * 8, o_ro = (o_ol + sizeof(OnlineList) + 7) & ~(size_t)7, o_io = o_ro + cc.rec_offs64.size() * 8,
                     o_rl = o_io + cc.in_offs64.size() * 8, o_il = o_rl + n_recl * 4, blob_bytes = o_il + n_inl * 4 + 8;
        int slot = 0;
        uint8_t* hb = ctx->open_slot(blob_bytes, &slot);
        if (!hb) return RV_E_NOMEM;
        uint64_t* dst = (uint64_t*)(hb + o_dst);  // per repetition: where this chunk's bytes of each vector go
        const uint64_t by_rec = (P->run.n_rec - P->pend_rec) / 8, by_in = (P->run.n_in - P->pend_in) / 8, by_pre = (P->run.n_pre - P->pend_pre) / 8;
        for (uint32_t r = 0; r < R; r++) {
            dst[0 * R + r] = P->offs[2 * R + r] + by_rec;
            dst[1 * R + r] = P->offs[4 * R + r] + by_in;
            dst[2 * R + r] = P->offs[5 * R + r] + 8 * P->run.n_rec64;
            dst[3 * R + r] = P->offs[6 * R + r] + 8 * P->run.n_corr64;
            dst[4 * R + r] = P->offs[7 * R + r] + 8 * P->run.n_in64;
            dst[5 * R + r] = 0;
        }
        OnlineList& ol = *(OnlineList*)(hb + o_ol);
        ol = P->ol;
        for (uint32_t k = 0; k < ol.n; k++) ol.dst[k] += by_pre;
        if (!cc.rec_offs64.empty()) memcpy(hb + o_ro, cc.rec_offs64.data(), cc.rec_offs64.size() * 8);
        if (!cc.in_offs64.empty()) memcpy(hb + o_io, cc.in_offs64.data(), cc.in_offs64.size() * 8);
        // item -> online row lists, the pending rows (now rows 0.. of this chunk's buffer) first
        uint32_t *rec_list = (uint32_t*)(hb + o_rl), *in_list = (uint32_t*)(hb + o_il);
        for (uint32_t i = 0; i < P->pend_rec; i++) rec_list[i] = i;
        if (!cc.rec_rows.empty()) memcpy(rec_list + P->pend_rec, cc.rec_rows.data(), cc.rec_rows.size() * 4);
        for (uint32_t i = 0; i < P->pend_in; i++) in_list[i] = P->pend_rec + i;
        if (!cc.in_rows.empty()) memcpy(in_list + P->pend_in, cc.in_rows.data(), cc.in_rows.size() * 4);
        const uint64_t rec_full = n_recl & ~(size_t)7, in_full = n_inl & ~(size_t)7, pre_full = cc.n_pre & ~(uint64_t)7;
        uint8_t* db = nullptr;
        if ((rc = take(blob_bytes, &db))) return rc;
        if ((rc = hip_code(hipMemcpyAsync(db, hb, blob_bytes, hipMemcpyHostToDevice, st), "opening tables")) ||
            (rc = hip_code(hipEventRecord(ctx->ev_open[slot], st), "opening tables")))
            return rc;
        uint64_t* d_dst = (uint64_t*)(db + o_dst);
        const uint32_t *d_rec_list = (const uint32_t*)(db + o_rl), *d_in_list = (const uint32_t*)(db + o_il);
        if (rec_full) launch_extract_bits(st, q.on(), d_rec_list, rec_full, NQ, 0, P->d_omit, d_dst + 0 * R, P->d_proof);
        if (in_full) launch_extract_bits(st, q.on(), d_in_list, in_full, NQ, 1, P->d_omit, d_dst + 1 * R, P->d_proof);
        if (pre_full) launch_extract_from_bits(st, q.pre(), pre_full, NQ, (const OnlineList*)(db + o_ol), P->d_proof);
        if (has64) {
            launch_extract64(st, q.on64(), q.pitch[TR_ON64], (const uint64_t*)(db + o_ro), cc.n_rec64, 1, R, P->d_omit, d_dst + 2 * R, P->d_proof);
            launch_extract64(st, q.pre64(), q.pitch[TR_PRE64], nullptr, cc.n_corr64, 0, R, P->d_omit, d_dst + 3 * R, P->d_proof);
            launch_extract64(st, q.on64(), q.pitch[TR_ON64], (const uint64_t*)(db + o_io), cc.n_in64, 0, R, P->d_omit, d_dst + 4 * R, P->d_proof);
        }
        // the items that do not fill a byte yet: their rows move to the pending buffers (one launch; the chunk's buffer and the
        // pending buffers are different allocations)
        const uint32_t nr = (uint32_t)(n_recl - rec_full), ni = (uint32_t)(n_inl - in_full), np = (uint32_t)(cc.n_pre - pre_full);
        CopySegs segs{};
        for (uint32_t i = 0; i < nr; i++) segs.add(q.on() + (size_t)rec_list[rec_full + i] * NQ, P->d_pend_rec + (size_t)i * NQ, NQ * 4);
        for (uint32_t i = 0; i < ni; i++) segs.add(q.on() + (size_t)in_list[in_full + i] * NQ, P->d_pend_in + (size_t)i * NQ, NQ * 4);
        if (np) segs.add(q.pre() + pre_full * (NQ / 2), P->d_pend_pre, np * (NQ / 2));
        cp.add(segs);
        P->pend_rec = nr;
        P->pend_in = ni;
        P->pend_pre = np;
        ctx->phase(-1);
        return RV_OK;
    }

    // the kept transcripts stay a chunk for every proof or for none
    void keep_for_all_or_none() {
        if (!p1 || !S->same_cuts) return;
        size_t n_kept = 0;
        for (rv_stream* Q : proofs) n_kept += Q->kept.count(first_op);
        if (n_kept && n_kept != proofs.size()) drop_all_kept();
    }

    // a chunk that ran leaves its error flags: read behind it now, or by the feed's one wait.  (A kept chunk ran nothing -- and
    // nothing on the host waits for its openings)
    int settle() {
        int rc = RV_OK;
        if (no_wait || (use_kept && !hashing && !ver && wit.dev))  // (a kept chunk runs nothing, but its device witness is still being digested)
            S->unsettled = true;
        else if (hashing || !use_kept)
            rc = stream_read_errs(proofs, "stream chunk");
        if (!rc) ctx->collect();
        t_gpu = Clock::now();
        return rc;
    }

    // The witness digest of a chunk fed from device memory: k_wit_sums over every proof's rows into the proofs' accumulators, keyed by
    // the ordinals the stream is at (count() advances them afterwards).  Also for a chunk served from kept transcripts, as the host loop.
    int digest_witness_on_device() {
        std::vector<uint64_t*> acc(proofs.size());
        for (size_t bi = 0; bi < proofs.size(); bi++) {
            rv_stream* Q = proofs[bi];
            if (!Q->d_wit_sum) {
                if (int rc = dalloc(ctx, 1, &Q->d_wit_sum)) return rc;
                if (int rc = hip_code(hipMemsetAsync(Q->d_wit_sum, 0, 8, st), "witness digest")) return rc;
            }
            acc[bi] = Q->d_wit_sum;
            Q->wit_dev_pass = true;
        }
        launch_wit_sums(st, wit.gf2, wit.stride2, cc.n_in, S->run.n_in, wit.z64, wit.stride64, cc.n_in64, S->run.n_in64, acc.data(), acc.size());
        return RV_OK;
    }

    // the counters: the same for every proof but the witness digest
    void count() {
        if (!ver && !wit.dev)
            for (size_t bi = 0; bi < proofs.size(); bi++) {  // (before the ordinals advance)
                rv_stream* Q = proofs[bi];
                Q->run.wit_hash += wit_digest(wit.gf2_of(bi), cc.n_in, Q->run.n_in, wit.z64_of(bi), cc.n_in64, Q->run.n_in64);
            }
        StreamTotals& t = S->run;
        t.n_ops += n_ops;
        t.ops_hash += digest;
        t.masks += cc.n_masks - cs.mask_phase;
        t.masks64 += cc.n_masks64 - cs.mask64_phase;
        // own events of this chunk (the compiled counters include the carried ones in front)
        t.n_on += cc.n_on - cs.on0;
        t.n_pre += cc.n_pre - cs.pre0;
        t.n_rec += cc.n_rec;
        t.n_in += cc.n_in;
        t.on_words64 += cc.on_words64 - cs.on_words64_0;
        t.pre_words64 += cc.pre_words64 - cs.pre_words64_0;
        t.n_rec64 += cc.n_rec64;
        t.n_corr64 += cc.n_corr64;
        t.n_in64 += cc.n_in64;
        t.levels += cc.info.levels;
        t.chunks++;
        for (size_t bi = 1; bi < proofs.size(); bi++) {
            rv_stream* Q = proofs[bi];
            const uint64_t wh = Q->run.wit_hash;
            Q->run = S->run;
            Q->run.wit_hash = wh;
        }
        used_gf2 = ver ? 0 : cc.n_in;  // (the verifier has no witness to advance in)
        used_z64 = ver ? 0 : cc.n_in64;
        lap_stats();
    }

    void lap_stats() {  // RV_STREAM_STATS: where the main thread's time goes, every 10 chunks
        static const bool stats = getenv("RV_STREAM_STATS") != nullptr;
        if (!stats) return;
        static double acc[6] = {0, 0, 0, 0, 0, 0};
        static int n_acc = 0;
        const Clock::time_point t[7] = {t_begin, t_reloc, t_up, t_alloc, t_issue, t_gpu, Clock::now()};
        for (int k = 0; k < 6; k++) acc[k] += std::chrono::duration<double>(t[k + 1] - t[k]).count();
        if (++n_acc % 10 == 0)
            fprintf(stderr, "[rv stream] %d chunks: relocate %.3f s, upload / plan %.3f s, buffers %.3f s, issue %.3f s, final sync %.3f s, counters %.3f s\n",
                    n_acc, acc[0], acc[1], acc[2], acc[3], acc[4], acc[5]);
    }
};

// pass 2: the chunk pass 1 compiled for the same ops (same first op, same length), if it was kept
static rv_circuit* stream_take_cached(rv_stream* S, uint64_t first_op, size_t n_ops, ChunkStart* carried, uint64_t* digest) {
    if (S->pass != 2) return nullptr;
    auto it = S->cache.find(first_op);
    if (it == S->cache.end() || it->second.n_ops != n_ops) return nullptr;
    rv_circuit* c = new rv_circuit();
    c->ctx = S->ctx;
    c->cc = std::move(it->second.cc);
    *carried = it->second.at;
    *digest = it->second.digest;
    S->cache_bytes -= std::min(S->cache_bytes, rv_stream::compiled_bytes(c->cc));
    S->cache.erase(it);
    return c;
}

// worker threads of a feed (RV_STREAM_THREADS; default: the host's cores, at most 6 -- measured on the 10^7-gate circuit:
// 2 threads 1.08 s, 4: 0.69, 6: 0.71, 8: 0.72, 16: 0.88; more threads slow the main thread's pageable uploads down
// (their allocations and the copies' page pinning meet in the kernel's address-space lock).  Letting the workers upload
// their pieces too (device-side relocation of the transcript offsets) was built and measured slower on every setting.)
static unsigned stream_threads() {
    if (const char* e = getenv("RV_STREAM_THREADS")) return (unsigned)std::max(atoi(e), 1);
    const unsigned hc = std::thread::hardware_concurrency();
    // (24 on a many-core host since the workers also copy their pieces into the page-locked ring -- 12 / 16 / 24 / 32 threads:
    // 134 / 126 / 118 / 110 ms for the 10^7-gate circuit; 12 while the main thread made that copy, and 6 was the optimum while
    // its pageable uploads met the workers' allocations in the address-space lock)
    return std::min(std::max(hc / 2, 1u), 24u);
}

// Where a feed is cut: every `full` ops -- except that a long feed of large chunks starts with pieces of 1/8, 1/4 and 1/2 of
// that (a piece is compiled by ONE worker thread at ~0.1 us per op; with all pieces the full size the GPU sat idle for the
// 0.1 s the first one takes).  The rule depends on the feed's length and the chunk size only, so pass 2 cuts the same feed
// the same way and finds pass 1's compiled pieces.  Piece i = ops [cut[i], cut[i + 1]).  (Also the streaming evaluator's.)
static std::vector<size_t> stream_cuts(size_t n_ops, size_t full) {
    std::vector<size_t> cut;
    size_t at = 0;
    cut.push_back(0);
    if (full >= ((size_t)1 << 16) && n_ops >= 4 * full)
        for (size_t part : {full / 8, full / 4, full / 2}) cut.push_back(at += part);
    while (at < n_ops) cut.push_back(at = std::min(n_ops, at + full));
    return cut;
}

// one piece of a feed on its way from the op array to the GPU
struct FeedPiece {
    size_t at = 0, n = 0;       // ops [at, at + n) of the feed
    bool predicted = false;     // ph2 / ph64 / want follow from counts over the pieces before it (else: from the stream when it is prepared)
    uint32_t ph2 = 0, ph64 = 0;
    ChunkStart want;            // the offsets the piece is expected to run at
    rv_circuit* c = nullptr;    // pass 1's compile out of the cache (checked against the ops fed now), then the piece as it will run
    uint64_t digest = 0;
    ChunkStart carried;         // the offsets c's arrays hold
    bool kept = false;          // pass 2: pass 1 kept this piece's transcripts (rv_stream::Kept) -- nothing of it is uploaded
    bool device = false;        // RV_COMPILE_DEVICE, all GF(2) (RV_COMPILE_DEVICE_Z64: no B2A; RV_COMPILE_DEVICE_B2A: any piece), not in pass 1's cache: c stays null until the main thread compiles it on the GPU
};

// A piece ready to run: pass 1's cached compile if its digest matches the ops fed now, else a fresh compile -- at the offsets the piece
// is expected to run at where they were predicted (no relocation pass afterwards; ChunkRun moves it by the difference, which is zero
// unless the prediction is off).  Runs on a worker thread, or inline right before the piece runs.
static int prepare_piece(const rv_stream* S, const FeedOps& fo, size_t i, uint64_t first_op, FeedPiece& p) {
    if (!p.predicted) p.ph2 = (uint32_t)(S->run.masks % 128), p.ph64 = (uint32_t)(S->run.masks64 % 2);
    const uint64_t dg = fo.digest(i, first_op);
    if (p.c && dg != p.digest) {  // same position and length, other ops: pass 1's compile is not this piece's (finish reports RV_E_ARG)
        rv_circuit_destroy(p.c);
        p.c = nullptr;
    }
    p.digest = dg;
    // (a piece whose transcripts pass 1 kept is compiled on the host as ever: ChunkRun::plan decides whether it runs at all)
    p.device = !p.c && !p.kept && fo.for_device(i, S->compile_flags);
    if (p.device) return RV_OK;
    if (!p.c) {
        p.carried = p.predicted ? p.want : ChunkStart();
        const PieceOnHost h(fo, i);
        if (h.rc()) return h.rc();
        if (int rc = stream_compile_piece(S, h.ops(), p.n, p.ph2, p.ph64, &p.c, p.predicted ? &p.want : nullptr)) return rc;
    }
    if (p.predicted) {
        relocate_to(p.c->cc, p.carried, p.want);
        set_carried(p.carried, p.want.pre0, p.want.on0, p.want.pre_words64_0, p.want.on_words64_0);
    }
    return RV_OK;
}

// The ring of page-locked slots (rv_ctx::h_ring): piece s goes into slot s % NS once piece s - NS has run -- a copy of ~13 MB per
// piece that used to sit on the main thread between two pieces' GPU work (1.2 of its ~2.2 ms per piece).  Returns NS (0: no ring).
static size_t feed_ring(rv_stream* S) {
    constexpr size_t NS_WANT = 6;
    rv_ctx* ctx = S->ctx;
    // a piece's arrays: its ops' gates and ordinal tables, PLUS the extra level that writes every wire it wrote back to the wire
    // store (up to one more gate per wire index: for the 10^7-gate circuit with recycled indices 2 x 10^5 gates = 9.6 MB beside the
    // 12 MB of a 2^18-op piece; sized without them, the slots were too small for every full-size piece and the main thread went
    // on copying: 0.16 -> 0.11 s per proof once a larger feed had grown the ring)
    const size_t wb2 = std::min<size_t>(S->gf2_wires, S->max_chunk_ops), wb64 = std::min<size_t>(S->z64_wires, S->max_chunk_ops);
    const size_t want_cap = ((S->max_chunk_ops * (sizeof(Gate) + 8) + wb2 * sizeof(Gate) + wb64 * sizeof(Gate64) + ((size_t)2 << 20)) + 0xFFFFF) & ~(size_t)0xFFFFF;
    if (want_cap > ((size_t)80 << 20)) return 0;
    if (ctx->h_ring_cap < want_cap || ctx->h_ring.size() < NS_WANT) {
        (void)hipStreamSynchronize(ctx->stream);
        for (uint8_t* p : ctx->h_ring) (void)hipHostFree(p);
        ctx->h_ring.clear();
        ctx->h_ring_cap = 0;
        for (hipEvent_t e : ctx->ring_ev)
            if (e) (void)hipEventDestroy(e);
        ctx->ring_ev.clear();
        for (size_t k = 0; k < NS_WANT; k++) {
            uint8_t* p = nullptr;
            if (hipHostMalloc((void**)&p, want_cap, hipHostMallocDefault) != hipSuccess) {
                (void)hipGetLastError();
                break;
            }
            ctx->h_ring.push_back(p);
        }
        ctx->h_ring_cap = want_cap;
    }
    while (ctx->ring_ev.size() < ctx->h_ring.size()) {
        hipEvent_t e = nullptr;
        if (hipEventCreateWithFlags(&e, hipEventDisableTiming) != hipSuccess) (void)hipGetLastError(), e = nullptr;
        ctx->ring_ev.push_back(e);
    }
    return ctx->h_ring.size();
}

// the mask and event counts of every piece of a feed (on a few threads: two passes over 10^7 ops on the main thread were 40 ms of a feed)
static rv_stream::FeedCounts feed_counts(rv_stream* S, const FeedOps& fo, const std::vector<size_t>& cut, uint64_t first_op) {
    // (rv_stream_same_cuts: pass 2 takes pass 1's counts of the same feed -- two passes over 240 MB of ops, 7 ms on 8 threads.
    // Other ops in pass 2 only make the predictions wrong: the pieces are then compiled again in place, and finish reports it)
    if (S->same_cuts && S->pass == 2) {
        auto it = S->feed_counts.find(first_op);
        if (it != S->feed_counts.end() && it->second.cut == cut) return it->second;
    }
    const size_t n_pieces = cut.size() - 1;
    rv_stream::FeedCounts k;
    k.cut = cut;
    k.cm2.resize(n_pieces), k.cm64.resize(n_pieces), k.cev.resize(n_pieces);
    // (a device feed has them from its kernel: nothing to spread over threads)
    const unsigned nt = fo.device ? 1u : (unsigned)std::min<size_t>({(size_t)16, n_pieces, (size_t)std::max(1u, std::thread::hardware_concurrency() / 2)});
    auto count = [&](unsigned t) {
        for (size_t i = t; i < n_pieces; i += nt) fo.counts(i, &k.cm2[i], &k.cm64[i], &k.cev[i]);
    };
    std::vector<std::thread> th;
    th.reserve(nt);
    try {
        for (unsigned t = 1; t < nt; t++) th.emplace_back(count, t);
    } catch (...) {
        for (auto& x : th) x.join();
        th.clear();
        for (unsigned t = 1; t < nt; t++) count(t);
    }
    count(0);
    for (auto& x : th) x.join();
    if (S->same_cuts && S->pass == 1) S->feed_counts[first_op] = k;
    return k;
}

// The pieces of a feed.  predict: every piece's ShareGen phases AND the carried transcript events it will find in front of its own
// follow from counts over the pieces before it, so the worker that compiles a piece also moves its transcript offsets (relocate_chunk:
// a pass over all its gates, 3 ms per 10^6 ops that the main thread used to spend between two chunks' GPU work).
static std::vector<FeedPiece> feed_pieces(rv_stream* S, const FeedOps& fo, const std::vector<size_t>& cut, bool predict) {
    const size_t n_pieces = cut.size() - 1;
    const uint64_t first_op = S->run.n_ops;
    std::vector<FeedPiece> pieces(n_pieces);
    rv_stream::FeedCounts fc;
    if (predict) fc = feed_counts(S, fo, cut, first_op);
    uint64_t m2 = S->run.masks, m64 = S->run.masks64;
    const bool tails = S->pass != 2;  // (the verifier's single pass carries unhashed tails like pass 1)
    uint64_t t[TR_KINDS];             // pass 1: unhashed tails
    for (int kind = 0; kind < TR_KINDS; kind++) t[kind] = S->tr[kind].tail;
    uint64_t pr = S->pend_rec, pi = S->pend_in, pp = S->pend_pre;  // pass 2: items short of a byte
    for (size_t i = 0; i < n_pieces; i++) {
        FeedPiece& p = pieces[i];
        p.at = cut[i];
        p.n = cut[i + 1] - cut[i];
        p.c = stream_take_cached(S, first_op + p.at, p.n, &p.carried, &p.digest);
        if (S->pass == 2) {
            auto it = S->kept.find(first_op + p.at);
            p.kept = it != S->kept.end() && it->second.n_ops == p.n;
        }
        if (!predict) continue;
        p.predicted = true;
        p.want.mask_phase = p.ph2 = (uint32_t)(m2 % 128);
        p.want.mask64_phase = p.ph64 = (uint32_t)(m64 % 2);
        m2 += fc.cm2[i];
        m64 += fc.cm64[i];
        const StreamEvents& ev = fc.cev[i];
        if (tails) {
            set_carried(p.want, t[TR_PRE], t[TR_ON], t[TR_PRE64], t[TR_ON64]);
            const uint64_t own[TR_KINDS] = {ev.pre2, ev.in2 + ev.rec2, ev.pre64, ev.on64};
            for (int kind = 0; kind < TR_KINDS; kind++) t[kind] = TR_KIND[kind].tail_of(t[kind] + own[kind]);
        } else {
            set_carried(p.want, pp, pr + pi, 0, 0);
            pr = (pr + ev.rec2) % 8, pi = (pi + ev.in2) % 8, pp = (pp + ev.pre2) % 8;
        }
    }
    return pieces;
}

// H: the caller's handle -- a single stream, or a batch whose members are fed witness b at wit_gf2 + b * n_gf2, wit_z64 + b * n_z64.
// The pieces are compiled ahead on worker threads (piece_pipe.h) and run in order; with one thread each is prepared right before it
// runs, unpredicted and unstaged.  ops_on_device: `ops` is in the memory of the stream's device (rv_stream_feed_device); what differs is
// behind FeedOps / PieceOnHost (feed_ops.inc).
// wit0: the feed's witness rows (host: rows n_gf2 / n_z64 apart; rv_stream_feed_wdev: the descriptor's, checked by its caller).
static int stream_feed_impl(rv_stream* H, const rv_op* ops, bool ops_on_device, size_t n_ops, const WitnessRows& wit0) {
    LibBusy busy_guard;  // (compile.h: the background unmapper keeps still while the GPU is driven)
    if (!H || (n_ops && !ops) || (ops_on_device && ((uintptr_t)ops & 7))) return RV_E_ARG;
    if (H->sticky) return H->sticky;
    const std::vector<rv_stream*> proofs = H->running();
    if (proofs.empty()) return RV_OK;  // (a verifier stream whose proof has the wrong shape: the answer is already `false`)
    rv_stream* S = proofs[0];          // (the host-side state of the feed: compiled-chunk cache, counts, pass)
    if (S->sticky) return H->sticky = S->sticky;
    H->fed = S->fed = true;
    HIPCHK(hipSetDevice(S->ctx->device));
    const bool stats = getenv("RV_STREAM_STATS") != nullptr;
    using Clock = std::chrono::steady_clock;
    auto secs = [](Clock::time_point a, Clock::time_point b) { return std::chrono::duration<double>(b - a).count(); };
    const auto t_feed0 = Clock::now();
    WitnessRows wit = wit0;
    const std::vector<size_t> cut = stream_cuts(n_ops, S->max_chunk_ops);  // piece i = ops [cut[i], cut[i + 1])
    const size_t n_pieces = cut.size() - 1;
    const unsigned n_threads = (unsigned)std::min<size_t>(stream_threads(), n_pieces);
    const bool ahead = n_threads > 1;
    const size_t NS = ahead ? feed_ring(S) : 0, slot_cap = S->ctx->h_ring_cap;
    const uint64_t first_op = S->run.n_ops;
    FeedOps fo(S->ctx, ops, ops_on_device && n_ops, cut);
    const auto t_sums0 = Clock::now();
    if (int rs = fo.load_sums(first_op, n_threads)) return S->sticky = H->sticky = rs;
    if (stats && fo.device)
        fprintf(stderr, "[rv stream] device feed: digest and counts of %zu pieces (%zu ops) in %.6f s (kernel, copy back, one wait)\n", n_pieces, n_ops,
                secs(t_sums0, Clock::now()));
    std::vector<FeedPiece> pieces = feed_pieces(S, fo, cut, ahead);
    // the second job of a worker: the next piece that is compiled, not yet with the main thread and whose slot is free goes into it
    size_t next_stage = 0;
    auto stage_pick = [&](const PiecePipe& pp) {
        while (next_stage < n_pieces && (pp.taken(next_stage) || pieces[next_stage].kept || (pp.ready(next_stage) && (pp.rc(next_stage) || !pieces[next_stage].c))))
            next_stage++;
        return next_stage < n_pieces && pp.ready(next_stage) && next_stage < pp.n_consumed() + NS ? next_stage++ : PiecePipe::NONE;
    };
    auto stage = [&](size_t i) {
        rv_circuit* c = pieces[i].c;
        if (circuit_stage_bytes(c->cc) > slot_cap) return;
        // (the copies out of the slot's previous piece may still be in flight: a chunk is not waited for)
        if (S->ctx->ring_ev[i % NS]) (void)hipEventSynchronize(S->ctx->ring_ev[i % NS]);
        circuit_stage(c, S->ctx->h_ring[i % NS], (int)(i % NS));
    };
    PiecePipe pipe(n_pieces, n_threads, RV_E_NOMEM, [&](size_t i) { return prepare_piece(S, fo, i, first_op, pieces[i]); },
                   NS ? PiecePipe::Pick(stage_pick) : PiecePipe::Pick(), stage);
    if (stats) fprintf(stderr, "[rv stream] feed set up (cuts, counts, cached pieces, %u workers) in %.3f s\n", n_threads, secs(t_feed0, Clock::now()));
    int rc = RV_OK;
    double t_wait = 0, t_run = 0, dev_laps[3] = {0, 0, 0};
    size_t n_dev = 0;
    // the host compile of a piece on this thread (what the device compiler handed back; a prediction that was off)
    auto compile_here = [&](size_t i, uint32_t ph2, uint32_t ph64, rv_circuit** out) {
        const PieceOnHost h(fo, i);
        return h.rc() ? h.rc() : stream_compile_piece(S, h.ops(), pieces[i].n, ph2, ph64, out);
    };
    for (size_t i = 0; i < n_pieces && !rc; i++) {
        FeedPiece& p = pieces[i];
        const auto t0 = Clock::now();
        rc = pipe.wait(i);
        rv_circuit* c = p.c;
        p.c = nullptr;
        if (rc) rv_circuit_destroy(c);
        if (!rc && !c && p.device) {
            // the device compile, here and in order on the context's stream: at the offsets the piece runs at (no relocation), its gate
            // records and ordinal tables left in HBM for circuit_upload
            const ChunkStart at = stream_chunk_start(S);
            c = new rv_circuit();
            c->ctx = S->ctx;
            DevCompileKeep kept;
            const int rd = fo.compile_on_device(i, S->z64_wires, S->gf2_wires, at, c->cc, &kept, stats ? dev_laps : nullptr, S->compile_flags);
            if (rd == RV_OK) {
                c->d_gates = kept.d_gates, c->d_rec_rows = kept.d_rec_rows, c->d_in_rows = kept.d_in_rows;
                c->d_gates64 = kept.d_gates64, c->d_rec_offs64 = kept.d_rec_offs64, c->d_in_offs64 = kept.d_in_offs64;
                c->dev_compiled = true;
                p.carried = at;
                p.ph2 = at.mask_phase, p.ph64 = at.mask64_phase;
                g_stream_device_chunks.fetch_add(1, std::memory_order_relaxed);
                n_dev++;
            } else {
                delete c;
                c = nullptr;
                p.carried = ChunkStart();
                p.ph2 = at.mask_phase, p.ph64 = at.mask64_phase;
                // (handed back -- an op-list error, a chain deeper than the round cap: the host compiler's result or error code)
                rc = rd == RV_COMPILE_FALLBACK ? compile_here(i, p.ph2, p.ph64, &c) : rd;
            }
        }
        if (!rc && (p.ph2 != (uint32_t)(S->run.masks % 128) || p.ph64 != (uint32_t)(S->run.masks64 % 2))) {
            // (cannot happen while count_masks agrees with the compiler; compile again in place rather than trust it)
            rv_circuit_destroy(c);
            c = nullptr;
            p.carried = ChunkStart();
            rc = compile_here(i, (uint32_t)(S->run.masks % 128), (uint32_t)(S->run.masks64 % 2), &c);
        }
        const auto t1 = Clock::now();
        if (!rc) {
            ChunkRun run(proofs, c, p.digest, p.n, wit);
            rc = run.run(p.carried);
            wit.advance(run.used_gf2, run.used_z64);
        }
        t_wait += secs(t0, t1);
        t_run += secs(t1, Clock::now());
        pipe.consumed(i, rc);
    }
    pipe.stop();
    for (FeedPiece& p : pieces)
        if (p.c) rv_circuit_destroy(p.c);  // compiled but never run (an earlier piece failed)
    if (stats)
        fprintf(stderr, "[rv stream] feed of %zu pieces on %u threads: %.3f s waiting for compiled pieces, %.3f s running them\n", n_pieces, n_threads,
                t_wait, t_run);
    if (stats && n_dev)
        fprintf(stderr, "[rv stream] device compile of %zu pieces (inside the waiting time): op upload %.3f s, compile %.3f s, host copy %.3f s\n", n_dev,
                dev_laps[0], dev_laps[1], dev_laps[2]);
    if (rc) S->sticky = H->sticky = rc;
    return rc;
}

// the one wait of a feed whose chunks were issued without one each (ChunkRun: no_wait): the error flags they left
static int stream_feed_settle(rv_stream* H) {
    if (!H) return RV_OK;
    const std::vector<rv_stream*> proofs = H->running();
    if (proofs.empty() || !proofs[0]->unsettled) return RV_OK;
    rv_stream* S = proofs[0];
    S->unsettled = false;
    const int rc = stream_read_errs(proofs, "stream feed");  // (the verifier: RV_DEV_ZERO_CHECK, read by the strict verifier at the end)
    if (rc) S->sticky = H->sticky = rc;
    return rc;
}

extern "C" int rv_stream_feed(rv_stream* S, const rv_op* ops, size_t n_ops, const uint8_t* wit_gf2, size_t n_gf2, const uint64_t* wit_z64,
                              size_t n_z64) {
    const int rc = guarded([&] { return stream_feed_impl(S, ops, false, n_ops, WitnessRows{wit_gf2, n_gf2, n_gf2, wit_z64, n_z64, n_z64}); });
    // (also after a failed feed: the caller's witness arrays and the ring slots may still feed copies)
    const int rs = stream_feed_settle(S);
    return rc ? rc : rs;
}

extern "C" int rv_stream_feed_device(rv_stream* S, const rv_op* d_ops, size_t n_ops, const uint8_t* wit_gf2, size_t n_gf2, const uint64_t* wit_z64,
                                     size_t n_z64) {
    const int rc = guarded([&] { return stream_feed_impl(S, d_ops, true, n_ops, WitnessRows{wit_gf2, n_gf2, n_gf2, wit_z64, n_z64, n_z64}); });
    const int rs = stream_feed_settle(S);  // (every read of d_ops has finished: the device compiles and the copies down are waited for)
    return rc ? rc : rs;
}

// the four stream digests of every repetition from the trees and the tails (S->d_dig: H_pre, H_on of GF(2), then of Z64)
static int stream_final_digests(rv_stream* S) {
    rv_ctx* ctx = S->ctx;
    constexpr uint32_t R = rv_stream::R;
    int rc;
    uint32_t* last = nullptr;
    if ((rc = dalloc(ctx, (size_t)R * 8, &last))) return rc;
    ctx->phase(RV_PH_HASH);
    // the streams' last chunks: what sits in the tails (an empty stream hashes as BLAKE3(""), root flag set)
    for (int kind = 0; kind < TR_KINDS; kind++) {
        const rv_stream::Transcript& T = S->tr[kind];
        TR_KIND[kind].hash(ctx->stream, T.d_tail, TR_KIND[kind].unit, T.tail, last, T.tree.chunks, T.tree.chunks == 0);
        inc_finish(ctx, T.tree, last, R, S->d_dig + (size_t)kind * R * 8);
    }
    ctx->phase(-1);
    ctx->release(last);  // (stream order keeps the arena's reuse behind the kernels that read it)
    return RV_OK;
}

// end of pass 1: the four stream digests, the per-repetition commitments, comm and the challenge -- all on the device
static int stream_commit_impl(rv_stream* S, uint8_t comm_out[RV_HASH_SIZE]) {
    if (!S || !S->bat.empty()) return RV_E_ARG;  // (a batch of several proofs commits with rv_stream_commit_batch)
    if (S->sticky) return S->sticky;
    if (S->pass != 1) return RV_E_ARG;
    rv_ctx* ctx = S->ctx;
    hipStream_t st = ctx->stream;
    constexpr uint32_t R = rv_stream::R, NQ = rv_stream::NQ;
    HIPCHK(hipSetDevice(ctx->device));
    int rc;
    const size_t DW = (size_t)R * 8;
    if ((rc = stream_final_digests(S))) return S->sticky = rc;
    ctx->phase(RV_PH_JOIN);
    launch_join(st, S->d_dig, S->d_dig + DW, S->d_dig + 2 * DW, S->d_dig + 3 * DW, R, S->d_h);
    ctx->phase(-1);
    // ---- layout of the proof from the totals, then Fiat-Shamir on the device
    S->tot = S->run;
    S->L = open_layout_of(S->tot.n_rec, S->tot.n_pre, S->tot.n_in, S->tot.n_rec64, S->tot.n_corr64, S->tot.n_in64, RV_ONLINE_REPS, RV_PREPROCESSING_REPS,
                          /*framed=*/true);
    constexpr size_t OL_WORDS = OPEN_OL_WORDS, FS_TAIL = OPEN_FS_TAIL;
    if ((rc = dalloc(ctx, R + FS_TAIL, &S->d_omit)) || (rc = dalloc(ctx, (size_t)8 * R + OL_WORDS, &S->d_offs)) ||
        (rc = dalloc(ctx, std::max<size_t>(S->L.total, 1), &S->d_proof)))
        return S->sticky = rc;
    HIPCHK(hipMemsetAsync(S->d_proof, 0, std::max<size_t>(S->L.total, 1), st));
    const FsLayout F = fs_layout_of(S->L, /*exact=*/true, S->d_proof);  // (a framed proof starts with comm)
    OnlineList* d_ol = (OnlineList*)(S->d_offs + (size_t)8 * R);
    ctx->phase(RV_PH_OPEN);
    launch_fs_challenge(st, S->d_h, F, 0, R, S->d_omit + R, S->d_omit, S->d_omit + R + 32, S->d_offs, d_ol, (uint32_t*)(S->d_omit + R + 32 + RV_TOTAL_REPS));
    ctx->phase(-1);
    S->offs.assign((size_t)8 * R + OL_WORDS, 0);
    uint8_t back[RV_TOTAL_REPS + 32];
    uint64_t wit_sum = 0;  // pass 1's device half of the witness digest (the layout above does not depend on it)
    HIPCHK(hipMemcpyAsync(S->offs.data(), S->d_offs, S->offs.size() * 8, hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(back, S->d_omit, sizeof back, hipMemcpyDeviceToHost, st));
    if (S->wit_dev_pass) HIPCHK(hipMemcpyAsync(&wit_sum, S->d_wit_sum, 8, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    S->tot.wit_hash += wit_sum;
    ctx->collect();
    memcpy(S->omit, back, RV_TOTAL_REPS);
    memcpy(S->comm, back + RV_TOTAL_REPS, 32);
    memcpy(&S->ol, &S->offs[(size_t)8 * R], sizeof S->ol);
    if (comm_out) memcpy(comm_out, S->comm, 32);
    // ---- pass 2 starts from the same initial state: zero wires, counters at zero
    if (S->d_rows) {
        HIPCHK(hipMemsetAsync(S->d_rows, 0, std::max<size_t>(S->gf2_wires, 1) * NQ * 4, st));
        HIPCHK(hipMemsetAsync(S->d_corr, 0, std::max<size_t>(S->gf2_wires, 1) * (NQ / 2), st));
    }
    if (S->d_wmask64) {
        HIPCHK(hipMemsetAsync(S->d_wmask64, 0, (1 + S->z64_wires) * (size_t)R * 64, st));
        HIPCHK(hipMemsetAsync(S->d_wcorr64, 0, (1 + S->z64_wires) * (size_t)R * 8, st));
    }
    HIPCHK(hipMemsetAsync(S->d_err, 0, sizeof(int), st));
    if (S->wit_dev_pass) HIPCHK(hipMemsetAsync(S->d_wit_sum, 0, 8, st));
    S->wit_dev_pass = false;
    S->run = StreamTotals{};
    S->pass = 2;
    return RV_OK;
}

extern "C" int rv_stream_same_cuts(rv_stream* S) {
    if (!S) return RV_E_ARG;
    if (S->sticky) return S->sticky;
    if (S->pass != 1) return RV_E_ARG;  // (a promise about pass 2, made during pass 1; a verifier stream has one pass)
    S->same_cuts = true;
    for (rv_stream* m : S->bat) m->same_cuts = true;
    return RV_OK;
}

extern "C" int rv_stream_commit(rv_stream* S, uint8_t comm[RV_HASH_SIZE]) {
    return guarded([&] { return stream_commit_impl(S, comm); });
}

// pass 2's device half of the witness digest into run.wit_hash (once: the accumulator starts again at zero)
static int stream_settle_wit_sum(rv_stream* S) {
    if (!S->wit_dev_pass) return RV_OK;
    uint64_t wit_sum = 0;
    HIPCHK(hipMemcpyAsync(&wit_sum, S->d_wit_sum, 8, hipMemcpyDeviceToHost, S->ctx->stream));
    HIPCHK(hipMemsetAsync(S->d_wit_sum, 0, 8, S->ctx->stream));
    HIPCHK(hipStreamSynchronize(S->ctx->stream));
    S->run.wit_hash += wit_sum;
    S->wit_dev_pass = false;
    return RV_OK;
}

// d_dst (null: the host form): the finished proof goes, counts and all, to the caller's device memory -- checked by the caller
static int stream_finish_impl(rv_stream* S, uint8_t** proof, size_t* proof_len, uint8_t* d_dst = nullptr) {
    if (!S || (!proof && !d_dst) || !proof_len) return RV_E_ARG;
    if (proof) *proof = nullptr;
    if (!d_dst) *proof_len = 0;
    if (!S->bat.empty()) return RV_E_ARG;  // (rv_stream_finish_batch)
    if (S->sticky) return S->sticky;
    if (S->pass != 2) return RV_E_ARG;
    rv_ctx* ctx = S->ctx;
    hipStream_t st = ctx->stream;
    constexpr uint32_t R = rv_stream::R, NQ = rv_stream::NQ;
    HIPCHK(hipSetDevice(ctx->device));
    int rc;
    if ((rc = stream_settle_wit_sum(S))) return S->sticky = rc;
    if (!(S->run == S->tot)) return S->sticky = RV_E_ARG;  // pass 2 was not fed what pass 1 was
    // ---- the vectors' last bytes: the pending (< 8) items, or the all-zero extra byte the reference always appends
    // (gf2/share.rs:126-138, gf2/recon.rs:217-229)
    std::vector<uint64_t> dst((size_t)2 * R, 0);
    for (uint32_t r = 0; r < R; r++) {
        dst[0 * R + r] = S->offs[2 * R + r] + (S->run.n_rec - S->pend_rec) / 8;
        dst[1 * R + r] = S->offs[4 * R + r] + (S->run.n_in - S->pend_in) / 8;
    }
    OnlineList ol = S->ol;
    for (uint32_t k = 0; k < ol.n; k++) ol.dst[k] += (S->run.n_pre - S->pend_pre) / 8;
    uint64_t* d_dst_rows = nullptr;
    OnlineList* d_ol = nullptr;
    if ((rc = dalloc(ctx, dst.size(), &d_dst_rows)) || (rc = dalloc(ctx, 1, &d_ol))) return S->sticky = rc;
    HIPCHK(hipMemcpyAsync(d_dst_rows, dst.data(), dst.size() * 8, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(d_ol, &ol, sizeof ol, hipMemcpyHostToDevice, st));
    ctx->phase(RV_PH_OPEN);
    launch_extract_bits(st, S->d_pend_rec, nullptr, S->pend_rec, NQ, 0, S->d_omit, d_dst_rows + 0 * R, S->d_proof);
    launch_extract_bits(st, S->d_pend_in, nullptr, S->pend_in, NQ, 1, S->d_omit, d_dst_rows + 1 * R, S->d_proof);
    launch_extract_from_bits(st, S->d_pend_pre, S->pend_pre, NQ, d_ol, S->d_proof);
    const size_t DW = (size_t)R * 8;
    launch_open_headers(st, R, S->d_omit, S->d_seeds, S->d_keys, S->d_dig + 1 * DW, S->d_dig + 3 * DW, S->d_offs, S->d_offs + R, S->L.l2r, S->L.l2c,
                        S->L.l2i, S->L.l64r, S->L.l64c, S->L.l64i, S->d_proof);
    ctx->phase(-1);
    if (d_dst) {  // the counts on the device, then the framed proof to where the caller wants it: no proof byte crosses to the host
        if (!launch_frame_counts(st, S->d_proof, 0, 1, S->L.len) || hipGetLastError() != hipSuccess) return S->sticky = RV_E_DEVICE;
        if (hipMemcpyAsync(d_dst, S->d_proof, S->L.total, hipMemcpyDeviceToDevice, st) != hipSuccess || hipStreamSynchronize(st) != hipSuccess)
            return S->sticky = hip_fail(hipGetLastError(), "stream proof D2D", __FILE__, __LINE__);
        ctx->collect();
        ctx->release(d_dst_rows);
        ctx->release(d_ol);
        *proof_len = S->L.total;
        S->sticky = RV_E_ARG;  // a finished stream takes no further calls (rv_stream_abort releases it)
        return RV_OK;
    }
    uint8_t* out = (uint8_t*)out_alloc(S->L.total);
    if (!out) return S->sticky = RV_E_NOMEM;
    stream_traffic(2, S->L.total);
    if (hipMemcpyAsync(out, S->d_proof, S->L.total, hipMemcpyDeviceToHost, st) != hipSuccess || hipStreamSynchronize(st) != hipSuccess) {
        rv_free(out);
        return S->sticky = hip_fail(hipGetLastError(), "stream proof D2H", __FILE__, __LINE__);
    }
    ctx->collect();
    ctx->release(d_dst_rows);
    ctx->release(d_ol);
    frame_counts_at(out, S->L.base);
    *proof = out;
    *proof_len = S->L.total;
    S->sticky = RV_E_ARG;  // a finished stream takes no further calls (rv_stream_abort releases it)
    return RV_OK;
}

extern "C" int rv_stream_finish(rv_stream* S, uint8_t** proof, size_t* proof_len) {
    return guarded([&] { return stream_finish_impl(S, proof, proof_len); });
}

extern "C" int rv_stream_get_info(const rv_stream* S, rv_stream_info* info) {
    if (!S || !info) return RV_E_ARG;
    memset(info, 0, sizeof *info);
    if (!S->bat.empty()) {  // a batch: the stream's counts (every proof's are the same) and the device bytes of all proofs together
        bool counted = false;
        for (const rv_stream* m : S->bat) {
            rv_stream_info mi;
            rv_stream_get_info(m, &mi);
            if (!counted && !m->format_bad) {
                counted = true;
                info->n_ops = mi.n_ops, info->chunks = mi.chunks, info->levels = mi.levels, info->gf2_masks = mi.gf2_masks, info->z64_masks = mi.z64_masks;
                info->gf2_muls = mi.gf2_muls, info->z64_muls = mi.z64_muls;
            }
            info->wire_store_bytes += mi.wire_store_bytes;
            info->peak_chunk_bytes += mi.peak_chunk_bytes;
            info->hash_state_bytes += mi.hash_state_bytes;
            info->proof_bytes += mi.proof_bytes;
            info->kept_mib += mi.kept_mib;
        }
        info->pass = (uint32_t)S->pass;
        return RV_OK;
    }
    const StreamTotals& t = S->pass == 1 ? S->run : S->tot;
    info->n_ops = t.n_ops;
    info->chunks = t.chunks;
    info->levels = t.levels;
    info->gf2_masks = t.masks;
    info->z64_masks = t.masks64;
    info->gf2_muls = t.n_pre;
    info->z64_muls = t.n_corr64;
    info->pass = (uint32_t)S->pass;
    info->kept_mib = (uint32_t)std::min<uint64_t>((S->kept_peak + ((1u << 20) - 1)) >> 20, 0xFFFFFFFFu);
    info->wire_store_bytes = (uint64_t)S->rows_cap * (rv_stream::NQ * 4 + rv_stream::NQ / 2) + (uint64_t)S->ssa64_cap * rv_stream::R * 72;
    info->peak_chunk_bytes = S->peak_bytes;
    for (int kind = 0; kind < TR_KINDS; kind++) info->hash_state_bytes += S->tr[kind].tree.node.size() * rv_stream::R * 32 + TR_KIND[kind].tail_bytes();
    info->proof_bytes = S->pass == 2 ? S->L.total : 0;
    return RV_OK;
}

// ------------------------------------------------------------------------------------
// The streaming VERIFIER: Proof::verify (/root/reference/src/proof/mod.rs:224-307) with the gate stream fed in pieces and
// device memory bounded like the streaming prover's (wire store + one chunk + the proof).  One pass: the omitted players
// are in the proof.  Every chunk runs in verify mode (7 of 8 PRGs and the supplied values for the opened repetitions,
// verifier/online.rs:25-183; all 8 and recomputed corrections for the others, verifier/preprocess.rs:17-79), its
// transcripts go into the same incremental BLAKE3 trees as the prover's first pass, and the end is rv_verify's end.
// ------------------------------------------------------------------------------------
// a verifier stream that runs nothing and answers `false`: rv_verify's answer for wrong repetition counts (proof/mod.rs:225-230),
// and a batch member whose proof is refused
static rv_stream* stream_dead_verifier(rv_ctx* ctx, const uint8_t* proof, size_t proof_len) {
    rv_stream* S = new rv_stream();
    S->ctx = ctx;
    S->pass = 3;
    S->format_bad = true;
    S->h_proof = proof;
    S->proof_len = proof_len;
    return S;
}

// The verifier's slot arrays (slot order: the 40 opened repetitions first) and the Z64 keys' scratch, every block on `tmp` until
// stream_verifier_arm hands it to a stream
static int stream_verifier_alloc(rv_ctx* ctx, DevSlotArrays& a, uint8_t*& d_keys64, std::vector<void*>& tmp) {
    constexpr uint32_t R = rv_stream::R, NQ = rv_stream::NQ;
    auto get = [&](size_t count, auto*& ptr) {
        const int rc = dalloc(ctx, count, &ptr);
        if (!rc) tmp.push_back(ptr);
        return rc;
    };
    int rc;
    if ((rc = get((size_t)R * 16, a.seeds)) || (rc = get(R, a.omit)) || (rc = get((size_t)R * 128, a.hkeys)) || (rc = get((size_t)R * 32, a.hco)) ||
        (rc = get((size_t)R * 32, a.hco64)) || (rc = get(NQ, a.keep)) || (rc = get(NQ, a.onm)) || (rc = get((size_t)6 * R, a.src)) ||
        (rc = get((size_t)R * 16, a.seeds64)) || (rc = get(R, a.omit64)) || (rc = get((size_t)R * 128, a.hkeys64)) || (rc = get(NQ, a.keep64)) ||
        (rc = get((size_t)6 * R, a.src64)) || (rc = get((size_t)R * 128, d_keys64)))
        return rc;
    return RV_OK;
}
// What both begins do once the arrays are filled in device memory: the eight arrays the chunks read now belong to the stream (and
// leave `tmp`), then the two transcripts' round keys; waits for the stream
static int stream_verifier_arm(rv_stream* S, const DevSlotArrays& a, uint8_t* d_keys64, std::vector<void*>& tmp) {
    constexpr uint32_t R = rv_stream::R, NQ = rv_stream::NQ;
    rv_ctx* ctx = S->ctx;
    hipStream_t st = ctx->stream;
    S->d_omit_v = a.omit, S->d_omit64_v = a.omit64, S->d_hco = a.hco, S->d_hco64 = a.hco64, S->d_keep = a.keep, S->d_keep64 = a.keep64, S->d_onm = a.onm,
    S->d_src = a.src;
    void* owned[] = {a.omit, a.omit64, a.hco, a.hco64, a.keep, a.keep64, a.onm, a.src};
    for (void* p : owned) tmp.erase(std::find(tmp.begin(), tmp.end(), p));
    if (int rc = dalloc(ctx, (size_t)RK_AREAS * 128 * NQ, &S->d_rk64)) return rc;
    // GF(2) transcript: the opened slots' keys are the proof's (omitted one zeroed, online.rs:101-113); the others came with the
    // prover's begin
    launch_overlay_rows(st, (uint32_t*)S->d_keys, (const uint32_t*)a.hkeys, S->d_omit_v, R, 32, 1);
    launch_key_schedule(st, S->d_keys, R * 8, S->d_rkbytes);
    launch_bitslice_rk(st, S->d_rkbytes, NQ, S->d_rk);
    // Z64 transcript: its own seeds / keys per repetition
    launch_verifier_keys(st, R, a.seeds64, a.hkeys64, S->d_omit64_v, d_keys64);
    launch_key_schedule(st, d_keys64, R * 8, S->d_rkbytes);
    launch_bitslice_rk(st, S->d_rkbytes, NQ, S->d_rk64);
    if (hipGetLastError() != hipSuccess || hipStreamSynchronize(st) != hipSuccess)
        return hip_fail(hipGetLastError(), "streaming verifier setup", __FILE__, __LINE__);
    return RV_OK;
}

static int stream_verify_begin_impl(rv_ctx* ctx, size_t z64_wires, size_t gf2_wires, const uint8_t* proof, size_t proof_len, size_t max_chunk_ops,
                                    rv_stream** out) {
    if (!ctx || !out || !proof) return RV_E_ARG;
    *out = nullptr;
    Parsed P;
    int rc = parse_proof(proof, proof_len, P);
    if (rc) return rc;
    constexpr uint32_t R = rv_stream::R, NQ = rv_stream::NQ;
    if (!format_ok(P)) {
        *out = stream_dead_verifier(ctx, proof, proof_len);
        return RV_OK;
    }
    // ---- the slots, as rv_verify_shard prepares them
    if ((rc = check_records_range(P, 0, R))) return rc;
    HostSlots H(R, true);
    fill_slots_range(P, proof, 0, R, 0, true, H.arrays());
    hipStream_t st = ctx->stream;
    rv_stream* S = nullptr;
    std::vector<void*> tmp;
    auto fail = [&](int code) {
        (void)hipStreamSynchronize(st);  // (the host vectors above leave scope)
        for (void* p : tmp) ctx->release(p);
        if (S) rv_stream_abort(S);
        return code;
    };
    DevSlotArrays a{};
    uint8_t* d_keys64 = nullptr;
    if ((rc = stream_verifier_alloc(ctx, a, d_keys64, tmp))) return fail(rc);
    // the prover's begin gives the stream its buffers and the GF(2) keys of the preprocessing slots (opened slots: overlaid below)
    if ((rc = stream_begin_impl(ctx, z64_wires, gf2_wires, H.seeds.data(), max_chunk_ops, &S))) return fail(rc);
    S->pass = 3;
    S->h_proof = proof;
    S->proof_len = proof_len;
    S->src64 = H.src64;
    S->sup_nq = supplied_nq(H.onm.data(), NQ);
    S->sup_r = supplied_r64(H.omit64.data(), R);
    if ((rc = dalloc(ctx, std::max<size_t>(proof_len, 1), &S->d_vproof))) return fail(rc);
    bool ok = true;
    auto up = [&](void* dst, const void* from, size_t n) { ok = ok && hipMemcpyAsync(dst, from, n, hipMemcpyHostToDevice, st) == hipSuccess; };
    up(S->d_vproof, proof, proof_len);
    stream_traffic(3, proof_len);
    up(a.omit, H.omit.data(), R);
    up(a.omit64, H.omit64.data(), R);
    up(a.hco, H.hco.data(), H.hco.size());
    up(a.hco64, H.hco64.data(), H.hco64.size());
    up(a.keep, H.keep.data(), (size_t)NQ * 4);
    up(a.keep64, H.keep64.data(), (size_t)NQ * 4);
    up(a.onm, H.onm.data(), (size_t)NQ * 4);
    up(a.src, H.src.data(), H.src.size() * 8);
    up(a.hkeys, H.hkeys.data(), H.hkeys.size());
    up(a.seeds64, H.seeds64.data(), H.seeds64.size());
    up(a.hkeys64, H.hkeys64.data(), H.hkeys64.size());
    if (!ok) return fail(hip_fail(hipGetLastError(), "streaming verifier setup", __FILE__, __LINE__));
    if ((rc = stream_verifier_arm(S, a, d_keys64, tmp))) return fail(rc);
    for (void* p : tmp) ctx->release(p);
    *out = S;
    return RV_OK;
}

extern "C" int rv_stream_verify_begin(rv_ctx* ctx, size_t z64_wires, size_t gf2_wires, const uint8_t* proof, size_t proof_len, size_t max_chunk_ops,
                                      rv_stream** out) {
    return guarded([&] { return stream_verify_begin_impl(ctx, z64_wires, gf2_wires, proof, proof_len, max_chunk_ops, out); });
}

static int stream_verify_finish_impl(rv_stream* S, uint32_t flags, int* ok) {
    if (!S || !ok || S->pass != 3 || !S->bat.empty()) return RV_E_ARG;
    if (!verify_flags_ok(flags)) return RV_E_ARG;
    *ok = 0;
    if (S->format_bad) return RV_OK;
    if (S->sticky) return S->sticky;
    rv_ctx* ctx = S->ctx;
    hipStream_t st = ctx->stream;
    constexpr uint32_t R = rv_stream::R;
    HIPCHK(hipSetDevice(ctx->device));
    int rc;
    if ((rc = stream_final_digests(S))) return S->sticky = rc;
    const size_t DW = (size_t)R * 8;
    // preprocessing slots: the online commitment is the one carried by the proof (preprocess.rs:55-57)
    launch_overlay_rows(st, S->d_dig + 1 * DW, (const uint32_t*)S->d_hco, S->d_omit_v, R, 8, 0);
    launch_overlay_rows(st, S->d_dig + 3 * DW, (const uint32_t*)S->d_hco64, S->d_omit_v, R, 8, 0);
    ctx->phase(RV_PH_JOIN);
    launch_join(st, S->d_dig, S->d_dig + DW, S->d_dig + 2 * DW, S->d_dig + 3 * DW, R, S->d_h);
    ctx->phase(-1);
    uint8_t digests[RV_TOTAL_REPS * 32];
    HIPCHK(hipMemcpyAsync(digests, S->d_h, sizeof digests, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    ctx->collect();
    ctx->prof.calls++;
    S->tot = S->run;
    if (S->proof_in_place) {  // verify_device_impl's end: rv_verify_finish_impl's decision from comm and the omit bytes the walk brought
        uint8_t omit[RV_TOTAL_REPS];
        *ok = digests_give_comm(S->dev_comm, digests, omit);
        if (verify_is_strict(flags)) {
            if (S->dev_flags & RV_DEV_ZERO_CHECK) *ok = 0;
            if (!records_omit_challenge(omit, S->dev_rec_omit, S->dev_rec_omit + RV_ONLINE_REPS)) *ok = 0;
        }
        return RV_OK;
    }
    return rv_verify_finish_impl(S->h_proof, S->proof_len, digests, flags, !(S->dev_flags & RV_DEV_ZERO_CHECK), ok);
}

extern "C" int rv_stream_verify_finish(rv_stream* S, uint32_t flags, int* ok) {
    return guarded([&] { return stream_verify_finish_impl(S, flags, ok); });
}

// Proof::verify with bounded device memory over an op array that already sits in host memory
extern "C" int rv_verify_streaming(rv_ctx* ctx, const rv_op* ops, size_t n_ops, size_t z64_wires, size_t gf2_wires, const uint8_t* proof, size_t proof_len,
                                   uint32_t flags, size_t max_chunk_ops, int* ok, rv_stream_info* info) {
    if (!ok) return RV_E_ARG;
    rv_stream* S = nullptr;
    int rc = rv_stream_verify_begin(ctx, z64_wires, gf2_wires, proof, proof_len, max_chunk_ops, &S);
    if (rc) return rc;
    rc = rv_stream_feed(S, ops, n_ops, nullptr, 0, nullptr, 0);
    if (!rc) rc = rv_stream_verify_finish(S, flags, ok);
    if (info) rv_stream_get_info(S, info);
    rv_stream_abort(S);
    return rc;
}

// both passes over an op array that is already in host memory (device memory stays bounded; the ops are walked twice)
extern "C" int rv_prove_streaming(rv_ctx* ctx, const rv_op* ops, size_t n_ops, size_t z64_wires, size_t gf2_wires, const uint8_t* wit_gf2, size_t n_gf2,
                                  const uint64_t* wit_z64, size_t n_z64, const uint8_t* seeds, size_t max_chunk_ops, uint8_t** proof, size_t* proof_len,
                                  rv_stream_info* info) {
    if (!proof || !proof_len) return RV_E_ARG;
    const bool stats = getenv("RV_STREAM_STATS") != nullptr;
    const auto t0 = std::chrono::steady_clock::now();
    auto lap = [&](const char* what) {
        if (stats) fprintf(stderr, "[rv stream] %-10s at %.3f s\n", what, std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count());
    };
    rv_stream* S = nullptr;
    int rc = rv_stream_begin(ctx, z64_wires, gf2_wires, seeds, max_chunk_ops, &S);
    if (rc) return rc;
    (void)rv_stream_same_cuts(S);  // (the same array, cut by the same rule in both passes)
    lap("begin");
    for (int pass = 0; pass < 2 && !rc; pass++) {
        rc = rv_stream_feed(S, ops, n_ops, wit_gf2, n_gf2, wit_z64, n_z64);
        lap(pass ? "feed 2" : "feed 1");
        if (!rc && pass == 0) rc = rv_stream_commit(S, nullptr);
        if (pass == 0) lap("commit");
    }
    if (!rc) rc = rv_stream_finish(S, proof, proof_len);
    lap("finish");
    if (info) rv_stream_get_info(S, info);
    rv_stream_abort(S);
    lap("released");
    return rc;
}

// ------------------------------------------------------------------------------------
// BATCHES: B witnesses (prover) or B proofs (verifier) of one statement over ONE fed op list.  The handle's members are complete
// single-proof streams; a feed compiles, relocates and uploads every chunk once and runs it for all members (ChunkRun),
// so B proofs cost one stream's host work -- the part that paces a streamed GF(2) proof -- plus B times the chunks' device work.
// ------------------------------------------------------------------------------------
// B wire stores must fit in half of what the device has free (plus what the context's arena holds idle): the batch is not split
static int stream_batch_fits(rv_ctx* ctx, size_t z64_wires, size_t gf2_wires, size_t batch) {
    constexpr uint64_t R = rv_stream::R, NQ = rv_stream::NQ;
    const long double one = (long double)gf2_wires * (NQ * 4 + NQ / 2) + (long double)(1 + z64_wires) * R * 72;
    size_t free_b = 0, total_b = 0;
    if (hipMemGetInfo(&free_b, &total_b) != hipSuccess) return hip_fail(hipGetLastError(), "hipMemGetInfo", __FILE__, __LINE__);
    if (one * (long double)batch > ((long double)free_b + (long double)ctx->cached_bytes) / 2) {
        g_last_error = "the batch's wire stores exceed half of the free device memory";
        return RV_E_NOMEM;
    }
    return RV_OK;
}

// A handle over `batch` member streams, member b begun by begin(b, &member); the first member that cannot begin ends them all
template <class Begin>
static int stream_batch_handle(rv_ctx* ctx, size_t z64_wires, size_t gf2_wires, size_t batch, int pass, Begin&& begin, rv_stream** out) {
    if (int rc = stream_batch_fits(ctx, z64_wires, gf2_wires, batch)) return rc;
    rv_stream* H = new rv_stream();
    H->ctx = ctx;
    H->z64_wires = z64_wires;
    H->gf2_wires = gf2_wires;
    H->pass = pass;
    for (size_t b = 0; b < batch; b++) {
        rv_stream* m = nullptr;
        if (int rc = begin(b, &m)) {
            rv_stream_abort(H);
            return rc;
        }
        H->bat.push_back(m);
    }
    *out = H;
    return RV_OK;
}

static int stream_begin_batch_impl(rv_ctx* ctx, size_t z64_wires, size_t gf2_wires, size_t batch, const uint8_t* seeds, size_t max_chunk_ops,
                                   rv_stream** out) {
    if (!ctx || !out) return RV_E_ARG;
    *out = nullptr;
    if (!batch) return RV_E_ARG;
    if (gf2_wires > 0x3FFFFFFFull || z64_wires > 0x3FFFFFFFull) return RV_E_UNSUPPORTED;
    HIPCHK(hipSetDevice(ctx->device));
    if (batch == 1) return stream_begin_impl(ctx, z64_wires, gf2_wires, seeds, max_chunk_ops, out);  // (a single stream, as rv_stream_begin)
    auto begin = [&](size_t b, rv_stream** m) {
        return stream_begin_impl(ctx, z64_wires, gf2_wires, seeds ? seeds + b * RV_TOTAL_REPS * RV_KEY_SIZE : nullptr, max_chunk_ops, m);
    };
    if (int rc = stream_batch_handle(ctx, z64_wires, gf2_wires, batch, 1, begin, out)) return rc;
    for (rv_stream* m : (*out)->bat) m->keep_cap /= batch;  // (RV_STREAM_KEEP_MB is the budget of the whole batch)
    return RV_OK;
}


extern "C" int rv_stream_begin_batch(rv_ctx* ctx, size_t z64_wires, size_t gf2_wires, size_t batch, const uint8_t* seeds, size_t max_chunk_ops,
                                     rv_stream** out) {
    return guarded([&] { return stream_begin_batch_impl(ctx, z64_wires, gf2_wires, batch, seeds, max_chunk_ops, out); });
}

static int stream_commit_batch_impl(rv_stream* S, uint8_t* comms) {
    if (!S) return RV_E_ARG;
    if (S->bat.empty()) return stream_commit_impl(S, comms);
    if (S->sticky) return S->sticky;
    if (S->pass != 1) return RV_E_ARG;
    HIPCHK(hipSetDevice(S->ctx->device));
    for (size_t b = 0; b < S->bat.size(); b++) {
        const int rc = stream_commit_impl(S->bat[b], comms ? comms + b * RV_HASH_SIZE : nullptr);
        if (rc) return S->sticky = rc;
    }
    S->pass = 2;
    return RV_OK;
}

extern "C" int rv_stream_commit_batch(rv_stream* S, uint8_t* comms) {
    return guarded([&] { return stream_commit_batch_impl(S, comms); });
}

static int stream_finish_batch_impl(rv_stream* S, uint8_t** proofs, size_t* proof_lens) {
    if (!S || !proofs || !proof_lens) return RV_E_ARG;
    if (S->bat.empty()) return stream_finish_impl(S, proofs, proof_lens);
    const size_t B = S->bat.size();
    for (size_t b = 0; b < B; b++) proofs[b] = nullptr, proof_lens[b] = 0;
    if (S->sticky) return S->sticky;
    if (S->pass != 2) return RV_E_ARG;
    HIPCHK(hipSetDevice(S->ctx->device));
    for (size_t b = 0; b < B; b++) {
        const int rc = stream_finish_impl(S->bat[b], &proofs[b], &proof_lens[b]);
        if (rc) {  // (pass 2 was not fed what pass 1 was, for this witness or the stream: no proof comes out)
            for (size_t k = 0; k < b; k++) rv_free(proofs[k]), proofs[k] = nullptr, proof_lens[k] = 0;
            return S->sticky = rc;
        }
    }
    S->sticky = RV_E_ARG;  // a finished stream takes no further calls (rv_stream_abort releases it)
    return RV_OK;
}

extern "C" int rv_stream_finish_batch(rv_stream* S, uint8_t** proofs, size_t* proof_lens) {
    return guarded([&] { return stream_finish_batch_impl(S, proofs, proof_lens); });
}

// one member of a verifier batch: a proof that cannot be parsed, or that the verifier's slots cannot take, is a member that runs
// nothing and answers `false` (rv_verify_batch's rule), like one with the wrong repetition counts
static int stream_verify_member(rv_ctx* ctx, size_t z64_wires, size_t gf2_wires, const uint8_t* proof, size_t proof_len, size_t max_chunk_ops,
                                rv_stream** out) {
    int rc = stream_verify_begin_impl(ctx, z64_wires, gf2_wires, proof, proof_len, max_chunk_ops, out);
    if (rc == RV_E_PROOF_MALFORMED) {
        *out = stream_dead_verifier(ctx, proof, proof_len);
        rc = RV_OK;
    }
    return rc;
}

static int stream_verify_begin_batch_impl(rv_ctx* ctx, size_t z64_wires, size_t gf2_wires, size_t batch, const uint8_t* const* proofs,
                                          const size_t* proof_lens, size_t max_chunk_ops, rv_stream** out) {
    if (!ctx || !out || !proofs || !proof_lens) return RV_E_ARG;
    *out = nullptr;
    if (!batch) return RV_E_ARG;
    for (size_t b = 0; b < batch; b++)
        if (!proofs[b]) return RV_E_ARG;
    if (gf2_wires > 0x3FFFFFFFull || z64_wires > 0x3FFFFFFFull) return RV_E_UNSUPPORTED;
    HIPCHK(hipSetDevice(ctx->device));
    auto begin = [&](size_t b, rv_stream** m) { return stream_verify_member(ctx, z64_wires, gf2_wires, proofs[b], proof_lens[b], max_chunk_ops, m); };
    if (batch == 1) return begin(0, out);
    return stream_batch_handle(ctx, z64_wires, gf2_wires, batch, 3, begin, out);
}


extern "C" int rv_stream_verify_begin_batch(rv_ctx* ctx, size_t z64_wires, size_t gf2_wires, size_t batch, const uint8_t* const* proofs,
                                            const size_t* proof_lens, size_t max_chunk_ops, rv_stream** out) {
    return guarded([&] { return stream_verify_begin_batch_impl(ctx, z64_wires, gf2_wires, batch, proofs, proof_lens, max_chunk_ops, out); });
}

static int stream_verify_finish_batch_impl(rv_stream* S, uint32_t flags, int* ok) {
    if (!S || !ok) return RV_E_ARG;
    if (S->bat.empty()) return stream_verify_finish_impl(S, flags, ok);
    if (S->pass != 3 || !verify_flags_ok(flags)) return RV_E_ARG;
    for (size_t b = 0; b < S->bat.size(); b++) ok[b] = 0;
    if (S->sticky) return S->sticky;
    for (size_t b = 0; b < S->bat.size(); b++) {
        const int rc = stream_verify_finish_impl(S->bat[b], flags, &ok[b]);
        if (rc == RV_E_PROOF_MALFORMED) {
            ok[b] = 0;  // (rejected alone)
        } else if (rc) {
            for (size_t k = 0; k < S->bat.size(); k++) ok[k] = 0;
            return S->sticky = rc;
        }
    }
    return RV_OK;
}

extern "C" int rv_stream_verify_finish_batch(rv_stream* S, uint32_t flags, int* ok) {
    return guarded([&] { return stream_verify_finish_batch_impl(S, flags, ok); });
}

// both passes of a batch over an op array that is already in host memory
extern "C" int rv_prove_streaming_batch(rv_ctx* ctx, const rv_op* ops, size_t n_ops, size_t z64_wires, size_t gf2_wires, size_t batch,
                                        const uint8_t* wit_gf2, size_t n_gf2, const uint64_t* wit_z64, size_t n_z64, const uint8_t* seeds,
                                        size_t max_chunk_ops, uint8_t** proofs, size_t* proof_lens, rv_stream_info* info) {
    if (!ctx || !proofs || !proof_lens || !batch) return RV_E_ARG;
    rv_stream* S = nullptr;
    int rc = rv_stream_begin_batch(ctx, z64_wires, gf2_wires, batch, seeds, max_chunk_ops, &S);
    if (rc) return rc;
    (void)rv_stream_same_cuts(S);  // (the same array, cut by the same rule in both passes)
    for (int pass = 0; pass < 2 && !rc; pass++) {
        rc = rv_stream_feed(S, ops, n_ops, wit_gf2, n_gf2, wit_z64, n_z64);
        if (!rc && pass == 0) rc = rv_stream_commit_batch(S, nullptr);
    }
    if (!rc) rc = rv_stream_finish_batch(S, proofs, proof_lens);
    if (info) rv_stream_get_info(S, info);
    rv_stream_abort(S);
    return rc;
}

extern "C" int rv_verify_streaming_batch(rv_ctx* ctx, const rv_op* ops, size_t n_ops, size_t z64_wires, size_t gf2_wires, size_t batch,
                                         const uint8_t* const* proofs, const size_t* proof_lens, uint32_t flags, size_t max_chunk_ops, int* ok,
                                         rv_stream_info* info) {
    if (!ctx || !proofs || !proof_lens || !ok || !batch) return RV_E_ARG;
    rv_stream* S = nullptr;
    int rc = rv_stream_verify_begin_batch(ctx, z64_wires, gf2_wires, batch, proofs, proof_lens, max_chunk_ops, &S);
    if (rc) return rc;
    rc = rv_stream_feed(S, ops, n_ops, nullptr, 0, nullptr, 0);
    if (!rc) rc = rv_stream_verify_finish_batch(S, flags, ok);
    if (info) rv_stream_get_info(S, info);
    rv_stream_abort(S);
    return rc;
}
