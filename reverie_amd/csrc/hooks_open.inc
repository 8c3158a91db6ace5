// Part of api.hip (#included there after hooks_b3.inc, whose recorder helper it uses): the Fiat-Shamir, record-head, framing and set-up
// kernels of open.hip, one production launch at a time on caller-supplied data (tests/test_gpu_open_heads.py).
//
// As in hooks.inc: the production launch_* function is called unchanged, every output buffer arrives pre-filled by the caller, is
// uploaded before the launch and comes back whole, and whatever a kernel relies on its callers for is checked on the host, RV_E_ARG
// before anything is allocated or launched.  Outputs that production keeps in host-mapped memory (the early path's mailbox, the error
// word of a small proof, k_store_words' destination) lie in a page of hipHostMallocMapped memory here too.
namespace {
constexpr size_t HOOK_PAGE_WORDS = 1024;
// one page of host-mapped memory for the process (allocating one per call cost more than the launches under test)
uint32_t* hook_mapped_page(uint32_t** dev) {
    static uint32_t* page = nullptr;
    if (!page && hipHostMalloc((void**)&page, HOOK_PAGE_WORDS * 4, hipHostMallocMapped) != hipSuccess) page = nullptr;
    if (!page || hipHostGetDevicePointer((void**)dev, page, 0) != hipSuccess) {
        (void)hipGetLastError();
        return nullptr;
    }
    return page;
}

// the heads of a shard's records inside a buffer of `bytes`: an opened repetition's record holds 153 + lr + lc + li bytes, another's 48
bool hook_heads_ok(uint32_t R, const uint8_t* omit, const uint64_t* off2, const uint64_t* off64, const uint64_t lens[6], uint64_t bytes) {
    if (!off2 || !off64) return false;
    for (int k = 0; k < 6; k++)
        if (lens[k] > HOOK_MAX) return false;
    const uint64_t rec2 = 153 + lens[0] + lens[1] + lens[2], rec64 = 153 + lens[3] + lens[4] + lens[5];
    for (uint32_t r = 0; r < R; r++) {
        const uint64_t n2 = omit[r] < 8 ? rec2 : 48, n64 = omit[r] < 8 ? rec64 : 48;
        if (off2[r] > bytes || n2 > bytes - off2[r] || off64[r] > bytes || n64 > bytes - off64[r]) return false;
    }
    return true;
}
}  // namespace

// launch_fs_challenge on digests [B][256][32] (B = batch, or 1 when batch is 0) for the shard (rep_begin, R).
//   layout[10]  FsLayout's base[4], sz2, sz64, l2r, l2c, l64r, l64c; framed as given (only the whole shard may be framed)
//   flags       bit 0: omit_all, bit 1: res, bit 2: comm2, bit 3: the mailbox are passed to the kernel (otherwise NULL)
// Outputs, B of each: comm [32], omit [R], omit_all [256], offs [8 R], ol [sizeof(OnlineList)] raw, res [2], comm2 [32]; mbox [128]
// words of the host-mapped page as production lays it out: word 0 the stamp (mbox_seq), from word 16 on the data.  batch >= 2: the
// call is recorded `batch` times on `batch` digest sets and replayed through k_many (no mailbox then: production's batches have none).
extern "C" int rv_hook_fs_challenge(rv_ctx* ctx, const uint8_t* digests, const uint64_t* layout, uint32_t framed, uint32_t rep_begin, uint32_t R, uint32_t flags,
                                    uint32_t mbox_seq, uint32_t batch, uint8_t* comm, uint8_t* omit, uint8_t* omit_all, uint64_t* offs, uint8_t* ol, uint32_t* res,
                                    uint8_t* comm2, uint32_t* mbox) {
    if (!ctx || !digests || !layout || !comm || !omit || !omit_all || !offs || !ol || !res || !comm2 || !mbox || framed > 1 || flags > 15 || !b3_hook_batch_ok(batch))
        return RV_E_ARG;
    // a shard as rv_shard_create takes it (the kernel indexes the whole map with rep_begin + r)
    if (!R || R % 8 || rep_begin % 8 || rep_begin > RV_TOTAL_REPS || R > RV_TOTAL_REPS - rep_begin) return RV_E_ARG;
    if (framed && (rep_begin != 0 || R != RV_TOTAL_REPS)) return RV_E_ARG;
    if ((flags & 8) && batch) return RV_E_ARG;
    for (int k = 0; k < 10; k++)
        if (layout[k] > (k < 4 ? HOOK_MAX << 8 : HOOK_MAX)) return RV_E_ARG;  // (section starts: 40 records of the largest size and more)
    HIPCHK(hipSetDevice(ctx->device));
    const size_t B = batch ? batch : 1, OL = sizeof(OnlineList);
    uint32_t *page = nullptr, *page_dev = nullptr;
    if ((flags & 8) && !(page = hook_mapped_page(&page_dev))) return RV_E_DEVICE;
    HookBufs bufs(ctx);
    uint8_t *d_h = nullptr, *d_comm = nullptr, *d_omit = nullptr, *d_all = nullptr, *d_ol = nullptr, *d_comm2 = nullptr;
    uint64_t* d_offs = nullptr;
    uint32_t* d_res = nullptr;
    int rc;
    if ((rc = bufs.up(digests, B * RV_TOTAL_REPS * 32, &d_h)) || (rc = bufs.up(comm, B * 32, &d_comm)) || (rc = bufs.up(omit, B * R, &d_omit)) ||
        (rc = bufs.up(omit_all, B * RV_TOTAL_REPS, &d_all)) || (rc = bufs.up(offs, B * 8 * R, &d_offs)) || (rc = bufs.up((const uint64_t*)ol, B * OL / 8, (uint64_t**)&d_ol)) ||
        (rc = bufs.up(res, B * 2, &d_res)) || (rc = bufs.up(comm2, B * 32, &d_comm2)))
        return rc;
    if (page) memcpy(page, mbox, 128 * 4);
    rc = b3_hook_issue(ctx, batch, [&](size_t b) {
        FsLayout L{};
        for (int k = 0; k < 4; k++) L.base[k] = layout[k];
        L.sz2 = layout[4], L.sz64 = layout[5], L.l2r = layout[6], L.l2c = layout[7], L.l64r = layout[8], L.l64c = layout[9];
        L.framed = framed;
        L.comm2 = (flags & 4) ? d_comm2 + b * 32 : nullptr;
        launch_fs_challenge(ctx->stream, d_h + b * RV_TOTAL_REPS * 32, L, rep_begin, R, d_comm + b * 32, d_omit + b * R, (flags & 1) ? d_all + b * RV_TOTAL_REPS : nullptr,
                            d_offs + b * 8 * R, (OnlineList*)(d_ol + b * OL), (flags & 2) ? d_res + b * 2 : nullptr, page ? page_dev + 16 : nullptr, page ? page_dev : nullptr,
                            mbox_seq);
    });
    if (rc) return rc;
    if ((rc = bufs.down(comm, d_comm, B * 32)) || (rc = bufs.down(omit, d_omit, B * R)) || (rc = bufs.down(omit_all, d_all, B * RV_TOTAL_REPS)) ||
        (rc = bufs.down(offs, d_offs, B * 8 * R)) || (rc = bufs.down(ol, d_ol, B * OL)) || (rc = bufs.down(res, d_res, B * 2)) || (rc = bufs.down(comm2, d_comm2, B * 32)))
        return rc;
    HIPCHK(hipStreamSynchronize(ctx->stream));
    if (page) memcpy(mbox, page, 128 * 4);
    return RV_OK;
}

// launch_open_headers: seeds [R][16], keys [R][128], on2 / on64 [R][8] u32 (the online transcripts' digests), off2 / off64 [R] the
// repetitions' records in `out`, lens[6] = l2r, l2c, l2i, l64r, l64c, l64i
extern "C" int rv_hook_open_headers(rv_ctx* ctx, uint32_t R, const uint8_t* omit, const uint8_t* seeds, const uint8_t* keys, const uint32_t* on2, const uint32_t* on64,
                                    const uint64_t* off2, const uint64_t* off64, const uint64_t* lens, uint8_t* out, uint64_t out_bytes) {
    if (!ctx || !seeds || !keys || !on2 || !on64 || !lens || !out || out_bytes > HOOK_MAX || !hook_map_ok(R, omit)) return RV_E_ARG;
    if (!hook_heads_ok(R, omit, off2, off64, lens, out_bytes)) return RV_E_ARG;
    HIPCHK(hipSetDevice(ctx->device));
    HookBufs bufs(ctx);
    uint8_t *d_omit = nullptr, *d_seeds = nullptr, *d_keys = nullptr, *d_out = nullptr;
    uint32_t *d_on2 = nullptr, *d_on64 = nullptr;
    uint64_t *d_off2 = nullptr, *d_off64 = nullptr;
    int rc;
    if ((rc = bufs.up(omit, (size_t)R, &d_omit)) || (rc = bufs.up(seeds, (size_t)R * 16, &d_seeds)) || (rc = bufs.up(keys, (size_t)R * 128, &d_keys)) ||
        (rc = bufs.up(on2, (size_t)R * 8, &d_on2)) || (rc = bufs.up(on64, (size_t)R * 8, &d_on64)) || (rc = bufs.up(off2, (size_t)R, &d_off2)) ||
        (rc = bufs.up(off64, (size_t)R, &d_off64)) || (rc = bufs.up(out, (size_t)out_bytes, &d_out)))
        return rc;
    launch_open_headers(ctx->stream, R, d_omit, d_seeds, d_keys, d_on2, d_on64, d_off2, d_off64, lens[0], lens[1], lens[2], lens[3], lens[4], lens[5], d_out);
    HIPCHK(hipGetLastError());
    if ((rc = bufs.down(out, d_out, (size_t)out_bytes))) return rc;
    HIPCHK(hipStreamSynchronize(ctx->stream));
    return RV_OK;
}

// launch_open_small: the heads as above with offs [8][R] (the challenge kernel's table) and the three GF(2) vectors -- rows rec_rows[0 .. n_rec)
// and in_rows[0 .. n_in) (NULL: 0, 1, ...) of stream [stream_rows][R/4] u32, and n_pre rows of the bit stream pre [n_pre][R/8] through the
// list ol (sizeof(OnlineList) raw bytes, as the challenge kernel leaves it).  flags bit 0: heads_inputs_only, bit 1: the host-mapped
// error word is passed (it receives err_src).  -> *taken (0: the launcher declined, nothing ran), tiles[3] (rec, corr, in), out, *err_word
extern "C" int rv_hook_open_small(rv_ctx* ctx, uint32_t R, const uint8_t* omit, const uint8_t* seeds, const uint8_t* keys, const uint32_t* on2, const uint32_t* on64,
                                  const uint64_t* offs, const uint64_t* lens, const uint32_t* stream, uint64_t stream_rows, const uint32_t* rec_rows, uint64_t n_rec,
                                  const uint8_t* pre, uint64_t n_pre, const uint32_t* in_rows, uint64_t n_in, const uint8_t* ol, uint32_t corr_rep_min, int err_src,
                                  uint32_t flags, uint8_t* out, uint64_t out_bytes, int* taken, uint32_t* tiles, int* err_word) {
    if (!ctx || !seeds || !keys || !on2 || !on64 || !offs || !lens || !ol || !out || !taken || !tiles || !err_word || flags > 3 || !hook_map_ok(R, omit)) return RV_E_ARG;
    if (out_bytes > HOOK_MAX || n_rec > HOOK_MAX || n_pre > HOOK_MAX || n_in > HOOK_MAX || stream_rows > HOOK_MAX || corr_rep_min > R) return RV_E_ARG;
    if ((stream_rows && !stream) || (n_pre && !pre)) return RV_E_ARG;
    if (!hook_heads_ok(R, omit, offs, offs + R, lens, out_bytes)) return RV_E_ARG;
    if (!hook_ranges_ok(R, omit, offs + 2 * (size_t)R, nullptr, n_rec / 8 + 1, out_bytes) || !hook_ranges_ok(R, omit, offs + 4 * (size_t)R, nullptr, n_in / 8 + 1, out_bytes))
        return RV_E_ARG;
    const std::pair<const uint32_t*, uint64_t> lists[2] = {{rec_rows, n_rec}, {in_rows, n_in}};
    for (const auto& l : lists) {
        if (l.first) {
            for (uint64_t i = 0; i < l.second; i++)
                if (l.first[i] >= stream_rows) return RV_E_ARG;
        } else if (l.second > stream_rows) {
            return RV_E_ARG;
        }
    }
    OnlineList list;
    memcpy(&list, ol, sizeof list);
    if (list.n > RV_ONLINE_REPS) return RV_E_ARG;
    for (uint32_t k = 0; k < list.n; k++) {
        if (list.rep[k] >= R) return RV_E_ARG;
        if (list.rep[k] >= corr_rep_min && (list.dst[k] > out_bytes || n_pre / 8 + 1 > out_bytes - list.dst[k])) return RV_E_ARG;
    }
    HIPCHK(hipSetDevice(ctx->device));
    uint32_t *page = nullptr, *page_dev = nullptr;
    if ((flags & 2) && !(page = hook_mapped_page(&page_dev))) return RV_E_DEVICE;
    const uint32_t NQ = R / 4;
    HookBufs bufs(ctx);
    uint8_t *d_omit = nullptr, *d_seeds = nullptr, *d_keys = nullptr, *d_pre = nullptr, *d_out = nullptr;
    uint32_t *d_on2 = nullptr, *d_on64 = nullptr, *d_stream = nullptr, *d_rec = nullptr, *d_in = nullptr;
    uint64_t *d_offs = nullptr, *d_ol = nullptr;
    int* d_err = nullptr;
    int rc;
    if ((rc = bufs.up(omit, (size_t)R, &d_omit)) || (rc = bufs.up(seeds, (size_t)R * 16, &d_seeds)) || (rc = bufs.up(keys, (size_t)R * 128, &d_keys)) ||
        (rc = bufs.up(on2, (size_t)R * 8, &d_on2)) || (rc = bufs.up(on64, (size_t)R * 8, &d_on64)) || (rc = bufs.up(offs, (size_t)8 * R, &d_offs)) ||
        (rc = bufs.up(stream, (size_t)stream_rows * NQ, &d_stream)) || (rec_rows && (rc = bufs.up(rec_rows, (size_t)n_rec, &d_rec))) ||
        (in_rows && (rc = bufs.up(in_rows, (size_t)n_in, &d_in))) || (rc = bufs.up(pre, (size_t)n_pre * (NQ / 2), &d_pre)) ||
        (rc = bufs.up((const uint64_t*)ol, sizeof(OnlineList) / 8, &d_ol)) || (rc = bufs.up(&err_src, 1, &d_err)) || (rc = bufs.up(out, (size_t)out_bytes, &d_out)))
        return rc;
    if (page) memcpy(page, err_word, sizeof(int));
    const bool t = launch_open_small(ctx->stream, R, d_omit, d_seeds, d_keys, d_on2, d_on64, d_offs, lens[0], lens[1], lens[2], lens[3], lens[4], lens[5], d_stream, d_rec,
                                     n_rec, d_pre, n_pre, d_in, n_in, NQ, (const OnlineList*)d_ol, corr_rep_min, d_out, d_err, page ? (int*)page_dev : nullptr, (flags & 1) != 0);
    HIPCHK(hipGetLastError());
    *taken = t ? 1 : 0;
    tiles[0] = extract_tile_bytes(n_rec), tiles[1] = extract_from_bits_tile_bytes(n_pre), tiles[2] = extract_tile_bytes(n_in);
    if ((rc = bufs.down(out, d_out, (size_t)out_bytes))) return rc;
    HIPCHK(hipStreamSynchronize(ctx->stream));
    if (page) memcpy(err_word, page, sizeof(int));
    return RV_OK;
}

// launch_frame_counts on `batch` proofs that lie `stride` bytes apart in out (out_bytes bytes); lens[4] the section lengths.
// *taken = 0: the launcher declined (no proof, an offset that is no multiple of 8) and nothing ran
extern "C" int rv_hook_frame_counts(rv_ctx* ctx, uint8_t* out, uint64_t out_bytes, uint64_t stride, uint32_t batch, const uint64_t* lens, int* taken) {
    if (!ctx || !out || !lens || !taken || out_bytes > HOOK_MAX || stride > HOOK_MAX || batch > (1u << 20)) return RV_E_ARG;
    uint64_t end = 32;
    for (int k = 0; k < 4; k++) {
        if (lens[k] > HOOK_MAX) return RV_E_ARG;
        end += 8 + (k < 3 ? lens[k] : 0);  // (the last count ends here: nothing is written into the fourth section)
    }
    if (batch && (end > out_bytes || (uint64_t)(batch - 1) * stride > out_bytes - end)) return RV_E_ARG;
    HIPCHK(hipSetDevice(ctx->device));
    HookBufs bufs(ctx);
    uint8_t* d_out = nullptr;
    int rc;
    if ((rc = bufs.up(out, (size_t)out_bytes, &d_out))) return rc;
    const size_t l[4] = {(size_t)lens[0], (size_t)lens[1], (size_t)lens[2], (size_t)lens[3]};
    *taken = launch_frame_counts(ctx->stream, d_out, stride, batch, l) ? 1 : 0;
    HIPCHK(hipGetLastError());
    if ((rc = bufs.down(out, d_out, (size_t)out_bytes))) return rc;
    HIPCHK(hipStreamSynchronize(ctx->stream));
    return RV_OK;
}

// ---- the verifier's and the prover's set-up kernels ----
// launch_overlay_rows: dst, src [R][row_words] u32
extern "C" int rv_hook_overlay_rows(rv_ctx* ctx, uint32_t* dst, const uint32_t* src, const uint8_t* omit, uint32_t R, uint32_t row_words, int want_online) {
    if (!ctx || !dst || !src || !row_words || row_words > 4096 || (want_online != 0 && want_online != 1) || !hook_map_ok(R, omit)) return RV_E_ARG;
    HIPCHK(hipSetDevice(ctx->device));
    HookBufs bufs(ctx);
    uint32_t *d_dst = nullptr, *d_src = nullptr;
    uint8_t* d_omit = nullptr;
    int rc;
    if ((rc = bufs.up(dst, (size_t)R * row_words, &d_dst)) || (rc = bufs.up(src, (size_t)R * row_words, &d_src)) || (rc = bufs.up(omit, (size_t)R, &d_omit))) return rc;
    launch_overlay_rows(ctx->stream, d_dst, d_src, d_omit, R, row_words, want_online);
    HIPCHK(hipGetLastError());
    if ((rc = bufs.down(dst, d_dst, (size_t)R * row_words))) return rc;
    HIPCHK(hipStreamSynchronize(ctx->stream));
    return RV_OK;
}

// launch_fill_digests: n_rows copies of digest[8] into dst (dst_words words)
extern "C" int rv_hook_fill_digests(rv_ctx* ctx, uint32_t* dst, uint64_t dst_words, uint32_t n_rows, const uint32_t* digest) {
    if (!ctx || !dst || !digest || !n_rows || n_rows > (1u << 20) || dst_words > HOOK_MAX || (uint64_t)n_rows * 8 > dst_words) return RV_E_ARG;
    HIPCHK(hipSetDevice(ctx->device));
    HookBufs bufs(ctx);
    uint32_t* d_dst = nullptr;
    int rc;
    if ((rc = bufs.up(dst, (size_t)dst_words, &d_dst))) return rc;
    launch_fill_digests(ctx->stream, d_dst, n_rows, digest);
    HIPCHK(hipGetLastError());
    if ((rc = bufs.down(dst, d_dst, (size_t)dst_words))) return rc;
    HIPCHK(hipStreamSynchronize(ctx->stream));
    return RV_OK;
}

// launch_shard_init: err [2] ints (the first is cleared), mask [mask_words] u32 and corr [corr_bytes] bytes of which the first n_mask_words /
// n_corr_bytes are cleared -- at most 64 each: the kernel is one workgroup of 64 threads without a loop --, fill (NULL or fill_words words:
// n_fill_rows copies of digest[8]), zero_byte (NULL or 8 bytes: the first is cleared)
extern "C" int rv_hook_shard_init(rv_ctx* ctx, int* err, uint32_t* mask, uint64_t mask_words, uint32_t n_mask_words, uint8_t* corr, uint64_t corr_bytes,
                                  uint32_t n_corr_bytes, uint32_t* fill, uint64_t fill_words, uint32_t n_fill_rows, const uint32_t* digest, uint8_t* zero_byte) {
    if (!ctx || !err || !mask || !corr || n_mask_words > 64 || n_corr_bytes > 64 || n_mask_words > mask_words || n_corr_bytes > corr_bytes) return RV_E_ARG;
    if (mask_words > HOOK_MAX || corr_bytes > HOOK_MAX || fill_words > HOOK_MAX || n_fill_rows > (1u << 20)) return RV_E_ARG;
    if (fill ? (!digest || (uint64_t)n_fill_rows * 8 > fill_words) : n_fill_rows != 0) return RV_E_ARG;
    HIPCHK(hipSetDevice(ctx->device));
    HookBufs bufs(ctx);
    int* d_err = nullptr;
    uint32_t *d_mask = nullptr, *d_fill = nullptr;
    uint8_t *d_corr = nullptr, *d_zero = nullptr;
    int rc;
    if ((rc = bufs.up(err, 2, &d_err)) || (rc = bufs.up(mask, (size_t)mask_words, &d_mask)) || (rc = bufs.up(corr, (size_t)corr_bytes, &d_corr)) ||
        (fill && (rc = bufs.up(fill, (size_t)fill_words, &d_fill))) || (zero_byte && (rc = bufs.up(zero_byte, 8, &d_zero))))
        return rc;
    launch_shard_init(ctx->stream, d_err, d_mask, n_mask_words, d_corr, n_corr_bytes, d_fill, n_fill_rows, digest, d_zero);
    HIPCHK(hipGetLastError());
    if ((rc = bufs.down(err, d_err, 2)) || (rc = bufs.down(mask, d_mask, (size_t)mask_words)) || (rc = bufs.down(corr, d_corr, (size_t)corr_bytes)) ||
        (fill && (rc = bufs.down(fill, d_fill, (size_t)fill_words))) || (zero_byte && (rc = bufs.down(zero_byte, d_zero, 8))))
        return rc;
    HIPCHK(hipStreamSynchronize(ctx->stream));
    return RV_OK;
}

// launch_store_words: src [n_words] into dst (dst_words words of the host-mapped page); with_err: the device error word (err_value) into
// *dst_err, a word of the same page
extern "C" int rv_hook_store_words(rv_ctx* ctx, const uint32_t* src, uint32_t n_words, uint32_t* dst, uint32_t dst_words, int err_value, int with_err, int* dst_err) {
    if (!ctx || !src || !dst || !dst_err || !n_words || n_words > dst_words || dst_words >= HOOK_PAGE_WORDS || (with_err != 0 && with_err != 1)) return RV_E_ARG;
    HIPCHK(hipSetDevice(ctx->device));
    uint32_t *page = nullptr, *page_dev = nullptr;
    if (!(page = hook_mapped_page(&page_dev))) return RV_E_DEVICE;
    HookBufs bufs(ctx);
    uint32_t* d_src = nullptr;
    int* d_err = nullptr;
    int rc;
    if ((rc = bufs.up(src, (size_t)n_words, &d_src)) || (rc = bufs.up(&err_value, 1, &d_err))) return rc;
    memcpy(page, dst, (size_t)dst_words * 4);
    memcpy(page + HOOK_PAGE_WORDS - 1, dst_err, 4);
    launch_store_words(ctx->stream, d_src, n_words, page_dev, with_err ? d_err : nullptr, (int*)(page_dev + HOOK_PAGE_WORDS - 1));
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(ctx->stream));
    memcpy(dst, page, (size_t)dst_words * 4);
    memcpy(dst_err, page + HOOK_PAGE_WORDS - 1, 4);
    return RV_OK;
}
