// Part of api.hip (#included there, one translation unit): the openings of a shard (ProverTranscript::extract, prover.rs:57-175) and the proof's assembly.

// layout of the opened shard in HBM: gf2_online | gf2_pre | z64_online | z64_pre
struct OpenLayout {
    uint64_t l2r, l2c, l2i, l64r, l64c, l64i, sz2, sz64;
    uint32_t n_on, n_pre;
    size_t len[4], base[4], total;
};

// From the six item counts (GF(2) broadcast / corrections / input bits, then the Z64 words) and the numbers of opened and unopened
// repetitions.  `framed`: leave room for the bincode framing of a whole Proof around the four sections
// (comm[32] | u64 n | gf2_online | u64 n | gf2_pre | u64 n | z64_online | u64 n | z64_pre), so a
// single-shard proof can be produced in its final layout on the device and copied out once
static OpenLayout open_layout_of(uint64_t n_rec, uint64_t n_pre, uint64_t n_in, uint64_t n_rec64, uint64_t n_corr64, uint64_t n_in64, uint32_t reps_on,
                                 uint32_t reps_pre, bool framed) {
    OpenLayout L{};
    // GF(2) vectors: 8 items per byte, plus the always-present extra chunk (SURVEY A.6)
    L.l2r = n_rec / 8 + 1;
    L.l2c = n_pre / 8 + 1;
    L.l2i = n_in / 8 + 1;
    // Z64 vectors: 8 bytes LE per item, no padding (z64/share.rs:42-48, z64/recon.rs:59-65)
    L.l64r = 8 * n_rec64;
    L.l64c = 8 * n_corr64;
    L.l64i = 8 * n_in64;
    L.sz2 = 1 + 128 + 24 + L.l2r + L.l2c + L.l2i;
    L.sz64 = 1 + 128 + 24 + L.l64r + L.l64c + L.l64i;
    L.n_on = reps_on, L.n_pre = reps_pre;
    L.len[0] = (size_t)L.n_on * L.sz2;
    L.len[1] = (size_t)L.n_pre * 48;
    L.len[2] = (size_t)L.n_on * L.sz64;
    L.len[3] = (size_t)L.n_pre * 48;
    size_t off = framed ? 32 : 0;
    for (int k = 0; k < 4; k++) {
        if (framed) off += 8;
        L.base[k] = off;
        off += L.len[k];
    }
    L.total = off;
    return L;
}
static OpenLayout open_layout(const Compiled& cc, const uint8_t* omit_local, uint32_t R, bool framed = false) {
    uint32_t n_on = 0;
    for (uint32_t r = 0; r < R; r++) n_on += omit_local[r] < 8;
    return open_layout_of(cc.n_rec, cc.n_pre, cc.n_in, cc.n_rec64, cc.n_corr64, cc.n_in64, n_on, R - n_on, framed);
}
// a whole proof, framed: any map with the 40 / 216 split gives the layout -- sizes do not depend on WHICH repetitions open
static OpenLayout whole_proof_layout(const Compiled& cc) {
    return open_layout_of(cc.n_rec, cc.n_pre, cc.n_in, cc.n_rec64, cc.n_corr64, cc.n_in64, RV_ONLINE_REPS, RV_PREPROCESSING_REPS, true);
}
// what k_fs_challenge needs of it.  exact: the shard opens 40 / 216 (a partial one gets its section starts on the device);
// comm2 (nullable): where a framed proof starts, for comm
static FsLayout fs_layout_of(const OpenLayout& L, bool exact, uint8_t* comm2) {
    FsLayout F{};
    for (int k = 0; k < 4; k++) F.base[k] = L.base[k];
    F.sz2 = L.sz2, F.sz64 = L.sz64, F.l2r = L.l2r, F.l2c = L.l2c, F.l64r = L.l64r, F.l64c = L.l64c;
    F.framed = exact ? 1u : 0u;
    F.comm2 = comm2;
    return F;
}

static void put_le64(uint8_t* p, uint64_t v) {
    for (int i = 0; i < 8; i++) p[i] = (uint8_t)(v >> (8 * i));
}
// the four repetition counts of a whole framed proof on the host: in front of sections that start at base[k] ...
static void frame_counts_at(uint8_t* out, const size_t base[4]) {
    const uint64_t counts[4] = {RV_ONLINE_REPS, RV_PREPROCESSING_REPS, RV_ONLINE_REPS, RV_PREPROCESSING_REPS};
    for (int k = 0; k < 4; k++) put_le64(out + base[k] - 8, counts[k]);
}
// ... or that follow comm one after the other with lens[k] bytes each
static void frame_counts_host(uint8_t* out, const size_t lens[4]) {
    size_t base[4], off = 32;
    for (int k = 0; k < 4; k++) {
        base[k] = off + 8;
        off += 8 + lens[k];
    }
    frame_counts_at(out, base);
}

extern "C" int rv_circuit_record_sizes(const rv_circuit* c, size_t* gf2_online_record, size_t* z64_online_record) {
    if (!c || !gf2_online_record || !z64_online_record) return RV_E_ARG;
    const OpenLayout L = whole_proof_layout(c->cc);
    *gf2_online_record = (size_t)L.sz2;
    *z64_online_record = (size_t)L.sz64;
    return RV_OK;
}

extern "C" int rv_shard_open_size(const rv_shard* s, const uint8_t omit[RV_TOTAL_REPS], size_t lens[4]) {
    if (!s || !omit || !lens) return RV_E_ARG;
    const OpenLayout L = open_layout(s->c->cc, omit + s->rep_begin, s->R);
    for (int k = 0; k < 4; k++) lens[k] = L.len[k];
    return RV_OK;
}

// What one openings call is given.  Unset fields mean: the challenge from the device, a block of the shard's own, unframed, the
// host waits and reads the result back, every corrections vector extracted.
struct OpenArgs {
    const uint8_t* omit = nullptr;      // the opening map [256] from the host; NULL: Fiat-Shamir on the device (k_fs_challenge) from the
                                        // shard's own digests -- only for a shard that holds all 256 repetitions -- or from d_all_h
    void* dst = nullptr;                // device memory for the openings
    bool framed = false;                // the framing of a whole Proof around the sections (open_layout_of)
    uint8_t* comm_out = nullptr;        // device Fiat-Shamir, read back: comm ...
    uint8_t* omit_out = nullptr;        // ... and the opening map
    bool no_sync = false;               // device Fiat-Shamir: nothing on the host depends on this proof yet; the caller synchronises
    const uint8_t* d_all_h = nullptr;   // device: all 256 digests (sharded proofs after the all-gather)
    // early corrections (ProveRun): the challenge is also published in this host-mapped mailbox -- sequence number fs_seq in word 0
    // once comm[32], the opening map [256] and {n_on, n_pre} stand from word 16 on -- and the GF(2) / Z64 corrections vectors of the
    // repetitions below corr2_rep_min / corr64_rep_min are NOT extracted (the host has them already)
    uint32_t* fs_mailbox = nullptr;
    uint32_t fs_seq = 0;
    uint32_t corr2_rep_min = 0, corr64_rep_min = 0;
};
struct OpenResult {
    void* d = nullptr;  // where the openings are (args.dst, or the shard's block)
    size_t lens[4] = {0, 0, 0, 0};
    size_t framed_total() const { return 32 + 4 * 8 + lens[0] + lens[1] + lens[2] + lens[3]; }
};
static int shard_open_impl(rv_shard* s, const OpenArgs& a, OpenResult* res);

extern "C" int rv_shard_open_device(rv_shard* s, const uint8_t omit[RV_TOTAL_REPS], void** dptr, size_t lens[4]) {
    if (!omit || !dptr || !lens) return RV_E_ARG;
    OpenArgs a;
    a.omit = omit;
    OpenResult res;
    const int rc = shard_open_impl(s, a, &res);
    if (rc) return rc;
    *dptr = res.d;
    for (int k = 0; k < 4; k++) lens[k] = res.lens[k];
    return RV_OK;
}

// the extern "C" forms that open into the caller's device memory and give back only the lengths
static int shard_open_to(rv_shard* s, const OpenArgs& a, size_t lens[4]) {
    if (!a.dst || !lens) return RV_E_ARG;
    OpenResult res;
    const int rc = shard_open_impl(s, a, &res);
    for (int k = 0; k < 4 && !rc; k++) lens[k] = res.lens[k];
    return rc;
}

extern "C" int rv_shard_open_into(rv_shard* s, const uint8_t omit[RV_TOTAL_REPS], void* dst_device, size_t lens[4]) {
    if (!omit) return RV_E_ARG;
    OpenArgs a;
    a.omit = omit;
    a.dst = dst_device;
    return shard_open_to(s, a, lens);
}

constexpr size_t OPEN_OL_WORDS = (sizeof(OnlineList) + 7) / 8;
// d_omit: [R] omit of the shard, then (device Fiat-Shamir) comm[32], the whole opening map [256], {n_on, n_pre}
constexpr size_t OPEN_FS_TAIL = 32 + RV_TOTAL_REPS + 8;

// The host's opening map as the kernels' table: off2, off64, gf2 rec/corr/in dst, z64 rec/corr/in dst ([8][R]); then the OnlineList
static std::vector<uint64_t> open_offsets_host(const OpenLayout& L, const uint8_t* om, uint32_t R) {
    std::vector<uint64_t> offs((size_t)8 * R + OPEN_OL_WORDS);
    uint32_t k_on = 0, k_pre = 0;
    OnlineList ol{};
    for (uint32_t r = 0; r < R; r++) {
        if (om[r] < 8) {
            offs[r] = L.base[0] + (uint64_t)k_on * L.sz2;
            offs[R + r] = L.base[2] + (uint64_t)k_on * L.sz64;
            offs[2 * R + r] = offs[r] + 137;
            offs[3 * R + r] = offs[r] + 145 + L.l2r;
            offs[4 * R + r] = offs[r] + 153 + L.l2r + L.l2c;
            offs[5 * R + r] = offs[R + r] + 137;
            offs[6 * R + r] = offs[R + r] + 145 + L.l64r;
            offs[7 * R + r] = offs[R + r] + 153 + L.l64r + L.l64c;
            if (ol.n < RV_ONLINE_REPS) {
                ol.rep[ol.n] = r;
                ol.dst[ol.n] = offs[3 * R + r];
                ol.n++;
            }
            k_on++;
        } else {
            offs[r] = L.base[1] + (uint64_t)k_pre * 48;
            offs[R + r] = L.base[3] + (uint64_t)k_pre * 48;
            k_pre++;
        }
    }
    memcpy(&offs[(size_t)8 * R], &ol, sizeof ol);
    return offs;
}

// k_open_small for a pure GF(2) shard: the heads and all three vectors (with err_dst the error word too), or the heads and the input
// vectors only.  false: nothing launched (Z64 vectors, a recorded batch, vectors too long for it: open.hip)
static bool open_small(rv_shard* s, const OpenLayout& L, const OnlineList* d_ol, uint32_t corr2_rep_min, uint8_t* d_out, int* err_dst, bool heads_inputs_only) {
    const Compiled& cc = s->c->cc;
    const size_t DW = (size_t)s->R * 8;
    if (cc.n_rec64 || cc.n_corr64 || cc.n_in64) return false;
    return launch_open_small(s->ctx->stream, s->R, s->d_omit, s->d_seeds, s->d_keys, s->d_dig + 1 * DW, s->d_dig + 3 * DW, s->d_offs, L.l2r, L.l2c, L.l2i, L.l64r, L.l64c,
                             L.l64i, s->d_on, s->c->d_rec_rows, cc.n_rec, s->d_pre, cc.n_pre, s->c->d_in_rows, cc.n_in, s->NQ, d_ol, corr2_rep_min, d_out, s->d_err,
                             err_dst, heads_inputs_only);
}

// The queueing: the challenge (or the host's map `om` and its table `offs`), then heads and vectors in the form open_small allows --
// counted for rv_hook_prove_schedule.  any_on: some repetition of the shard opens (device Fiat-Shamir: not known on the host yet)
static int open_queue(rv_shard* s, const OpenArgs& a, const OpenLayout& L, const uint8_t* om, const std::vector<uint64_t>& offs, bool any_on, uint8_t* d_out) {
    rv_ctx* ctx = s->ctx;
    const Compiled& cc = s->c->cc;
    const size_t DW = (size_t)s->R * 8;
    const OnlineList* d_ol = (const OnlineList*)(s->d_offs + (size_t)8 * s->R);
    ctx->phase(RV_PH_OPEN);
    if (!om) {
        const bool whole = s->rep_begin == 0 && s->R == RV_TOTAL_REPS;
        // (fs_mailbox: the kernel itself leaves comm, the opening map and the counts in the host-mapped mailbox and stamps it)
        launch_fs_challenge(ctx->stream, a.d_all_h ? a.d_all_h : s->d_h, fs_layout_of(L, whole, a.framed ? d_out : nullptr), s->rep_begin, s->R, s->d_omit + s->R,
                            s->d_omit, s->d_omit + s->R + 32, s->d_offs, (OnlineList*)d_ol, (uint32_t*)(s->d_omit + s->R + 32 + RV_TOTAL_REPS),
                            a.fs_mailbox ? a.fs_mailbox + 16 : nullptr, a.fs_mailbox, a.fs_seq);
        ctx->count();
    } else {
        HIPCHK(hipMemcpyAsync(s->d_omit, om, s->R, hipMemcpyHostToDevice, ctx->stream));
        HIPCHK(hipMemcpyAsync(s->d_offs, offs.data(), offs.size() * 8, hipMemcpyHostToDevice, ctx->stream));
    }
    ctx->count(any_on ? 4 : 1);
    // one small GF(2) proof: heads and vectors in ONE launch
    const bool fused = any_on && !s->od_out && open_small(s, L, d_ol, a.corr2_rep_min, d_out, s->err_dst_mapped, false);
    s->err_word_sent = fused && s->err_dst_mapped;
    // a large GF(2) proof: at least the heads and the input vectors together (its long vectors below)
    const bool heads_in = !fused && any_on && open_small(s, L, d_ol, a.corr2_rep_min, d_out, nullptr, true);
    prove_counted(fused ? PS_OPEN_ONE : heads_in ? PS_OPEN_HEADS_INPUTS : PS_OPEN_SEPARATE), prove_counted(PS_OPEN_ERR_WORD, s->err_word_sent);
    if (!fused && !heads_in)
        launch_open_headers(ctx->stream, s->R, s->d_omit, s->d_seeds, s->d_keys, s->d_dig + 1 * DW, s->d_dig + 3 * DW, s->d_offs, s->d_offs + s->R, L.l2r, L.l2c,
                            L.l2i, L.l64r, L.l64c, L.l64i, d_out);
    if (any_on && !fused) {
        launch_extract_bits(ctx->stream, s->d_on, s->c->d_rec_rows, cc.n_rec, s->NQ, 0, s->d_omit, s->d_offs + 2 * s->R, d_out, s->od_out, s->od_n_direct);
        if (a.corr2_rep_min < s->R) launch_extract_from_bits(ctx->stream, s->d_pre, cc.n_pre, s->NQ, d_ol, d_out, a.corr2_rep_min);
        if (!heads_in) launch_extract_bits(ctx->stream, s->d_on, s->c->d_in_rows, cc.n_in, s->NQ, 1, s->d_omit, s->d_offs + 4 * s->R, d_out);
        launch_extract64(ctx->stream, s->d_on64, cc.on_words64, s->c->d_rec_offs64, cc.n_rec64, 1, s->R, s->d_omit, s->d_offs + 5 * s->R, d_out, d_ol);
        launch_extract64(ctx->stream, s->d_pre64, cc.pre_words64, nullptr, cc.n_corr64, 0, s->R, s->d_omit, s->d_offs + 6 * s->R, d_out, d_ol, a.corr64_rep_min);
        launch_extract64(ctx->stream, s->d_on64, cc.on_words64, s->c->d_in_offs64, cc.n_in64, 0, s->R, s->d_omit, s->d_offs + 7 * s->R, d_out, d_ol);
    }
    HIPCHK(hipGetLastError());
    ctx->phase(-1);
    return RV_OK;
}

// The result: the section lengths -- the layout's, or, read back after device Fiat-Shamir, the challenge's -- with comm and the map
// where asked for.  The host waits for the stream unless no_sync says the caller will.
static int open_result(rv_shard* s, const OpenArgs& a, const OpenLayout& L, uint8_t* d_out, OpenResult* res) {
    rv_ctx* ctx = s->ctx;
    res->d = d_out;
    for (int k = 0; k < 4; k++) res->lens[k] = L.len[k];
    if (!a.omit && a.no_sync) return RV_OK;
    if (a.omit) {
        HIPCHK(hipStreamSynchronize(ctx->stream));  // (the host's offset table must outlive its asynchronous copy)
        ctx->collect();
        return RV_OK;
    }
    uint8_t back[OPEN_FS_TAIL];
    HIPCHK(hipMemcpyAsync(back, s->d_omit + s->R, sizeof back, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    if (a.comm_out) memcpy(a.comm_out, back, 32);
    if (a.omit_out) memcpy(a.omit_out, back + 32, RV_TOTAL_REPS);
    uint32_t cnt[2];
    memcpy(cnt, back + 32 + RV_TOTAL_REPS, sizeof cnt);
    ctx->collect();
    res->lens[0] = (size_t)cnt[0] * L.sz2;
    res->lens[1] = (size_t)cnt[1] * 48;
    res->lens[2] = (size_t)cnt[0] * L.sz64;
    res->lens[3] = (size_t)cnt[1] * 48;
    return RV_OK;
}

static int shard_open_impl(rv_shard* s, const OpenArgs& a, OpenResult* res) {
    if (!s || !res) return RV_E_ARG;
    if (a.fs_mailbox && a.omit) return RV_E_ARG;
    rv_ctx* ctx = s->ctx;
    HIPCHK(hipSetDevice(ctx->device));
    const bool self = a.omit == nullptr;
    const bool whole = s->rep_begin == 0 && s->R == RV_TOTAL_REPS;
    // device Fiat-Shamir needs all 256 digests: the shard's own when it holds every repetition, else the gathered ones;
    // a partial shard's output size depends on the challenge, so the caller provides the buffer (worst case, see header)
    if (self && !whole && (!a.d_all_h || !a.dst || a.framed || a.no_sync)) return RV_E_ARG;
    const uint8_t* om = self ? nullptr : a.omit + s->rep_begin;
    for (uint32_t r = 0; r < s->R && om; r++)
        if (om[r] > 8) return RV_E_ARG;
    const Compiled& cc = s->c->cc;
    // (device mode: the canonical split -- the first 40 repetitions of the shard open -- gives the sizes)
    const uint32_t canon_on = std::min<uint32_t>(RV_ONLINE_REPS, s->R);
    const OpenLayout L = self ? open_layout_of(cc.n_rec, cc.n_pre, cc.n_in, cc.n_rec64, cc.n_corr64, cc.n_in64, canon_on, s->R - canon_on, a.framed)
                              : open_layout(cc, om, s->R, a.framed);
    const std::vector<uint64_t> offs = self ? std::vector<uint64_t>() : open_offsets_host(L, om, s->R);
    int rc;
    ctx->release(s->d_omit);
    ctx->release(s->d_offs);
    ctx->release(s->d_out);
    s->d_omit = nullptr;
    s->d_offs = nullptr;
    s->d_out = nullptr;
    if ((rc = dalloc(ctx, s->R + OPEN_FS_TAIL, &s->d_omit)) || (rc = dalloc(ctx, (size_t)8 * s->R + OPEN_OL_WORDS, &s->d_offs))) return rc;
    uint8_t* d_out = (uint8_t*)a.dst;
    if (!d_out) {
        if ((rc = dalloc(ctx, std::max<size_t>(L.total, 1), &s->d_out))) return rc;
        d_out = s->d_out;
    }
    if ((rc = open_queue(s, a, L, om, offs, self || L.n_on, d_out))) return rc;
    return open_result(s, a, L, d_out, res);
}

extern "C" int rv_shard_open_self(rv_shard* s, void* dst_device, uint8_t comm[RV_HASH_SIZE], uint8_t omit[RV_TOTAL_REPS],
                                  size_t lens[4]) {
    if (!comm || !omit) return RV_E_ARG;
    OpenArgs a;
    a.dst = dst_device;
    a.comm_out = comm;
    a.omit_out = omit;
    return shard_open_to(s, a, lens);
}

extern "C" int rv_shard_open_gathered(rv_shard* s, const void* all_digests_device, void* dst_device, uint8_t comm[RV_HASH_SIZE],
                                      uint8_t omit[RV_TOTAL_REPS], size_t lens[4]) {
    if (!all_digests_device || !comm || !omit) return RV_E_ARG;
    OpenArgs a;
    a.dst = dst_device;
    a.comm_out = comm;
    a.omit_out = omit;
    a.d_all_h = (const uint8_t*)all_digests_device;
    return shard_open_to(s, a, lens);
}

extern "C" int rv_shard_open(rv_shard* s, const uint8_t omit[RV_TOTAL_REPS], rv_shard_parts* parts) {
    if (!parts) return RV_E_ARG;
    memset(parts, 0, sizeof *parts);
    void* d = nullptr;
    size_t lens[4];
    int rc = rv_shard_open_device(s, omit, &d, lens);
    if (rc) return rc;
    uint8_t** dst[4] = {&parts->gf2_online, &parts->gf2_pre, &parts->z64_online, &parts->z64_pre};
    size_t* dl[4] = {&parts->gf2_online_len, &parts->gf2_pre_len, &parts->z64_online_len, &parts->z64_pre_len};
    size_t off = 0;
    for (int k = 0; k < 4; k++) {
        *dst[k] = (uint8_t*)malloc(lens[k] ? lens[k] : 1);
        if (!*dst[k]) return RV_E_NOMEM;
        if (lens[k]) HIPCHK(hipMemcpyAsync(*dst[k], (uint8_t*)d + off, lens[k], hipMemcpyDeviceToHost, s->ctx->stream));
        *dl[k] = lens[k];
        off += lens[k];
    }
    HIPCHK(hipStreamSynchronize(s->ctx->stream));
    const uint8_t* om = omit + s->rep_begin;
    for (uint32_t r = 0; r < s->R; r++) (om[r] < 8 ? parts->n_online : parts->n_pre)++;
    return RV_OK;
}

extern "C" int rv_assemble_proof(const uint8_t comm[RV_HASH_SIZE], const rv_shard_parts* parts, size_t n_parts, uint8_t** proof,
                                 size_t* proof_len) {
    if (!comm || !parts || !proof || !proof_len) return RV_E_ARG;
    size_t total = 32 + 4 * 8;
    uint64_t n_on = 0, n_pre = 0;
    for (size_t i = 0; i < n_parts; i++) {
        total += parts[i].gf2_online_len + parts[i].gf2_pre_len + parts[i].z64_online_len + parts[i].z64_pre_len;
        n_on += parts[i].n_online;
        n_pre += parts[i].n_pre;
    }
    uint8_t* out = (uint8_t*)malloc(total);
    if (!out) return RV_E_NOMEM;
    uint8_t* w = out;
    memcpy(w, comm, 32);
    w += 32;
    // Proof { comm, gf2: ProofSingle, z64: ProofSingle }, ProofSingle { online: Vec, preprocessing: Vec }
    for (int dom = 0; dom < 2; dom++) {
        put_le64(w, n_on);
        w += 8;
        for (size_t i = 0; i < n_parts; i++) {
            const uint8_t* p = dom == 0 ? parts[i].gf2_online : parts[i].z64_online;
            const size_t l = dom == 0 ? parts[i].gf2_online_len : parts[i].z64_online_len;
            if (l) memcpy(w, p, l);
            w += l;
        }
        put_le64(w, n_pre);
        w += 8;
        for (size_t i = 0; i < n_parts; i++) {
            const uint8_t* p = dom == 0 ? parts[i].gf2_pre : parts[i].z64_pre;
            const size_t l = dom == 0 ? parts[i].gf2_pre_len : parts[i].z64_pre_len;
            if (l) memcpy(w, p, l);
            w += l;
        }
    }
    *proof = out;
    *proof_len = total;
    return RV_OK;
}
