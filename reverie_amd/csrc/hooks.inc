// Part of api.hip (#included there, one translation unit): parity-test hooks (rv_hook_*).

// ------------------------------------------------------------------------------------
// parity-test hooks
// ------------------------------------------------------------------------------------
extern "C" int rv_hook_expand_seed(rv_ctx* ctx, const uint8_t* seeds, size_t n, uint8_t* keys) {
    if (!ctx || !seeds || !keys || !n) return RV_E_ARG;
    HIPCHK(hipSetDevice(ctx->device));
    uint8_t *ds = nullptr, *dk = nullptr;
    int rc;
    if ((rc = dalloc(ctx, n * 16, &ds)) || (rc = dalloc(ctx, n * 128, &dk))) return rc;
    HIPCHK(hipMemcpyAsync(ds, seeds, n * 16, hipMemcpyHostToDevice, ctx->stream));
    launch_expand_seeds(ctx->stream, ds, (uint32_t)n, dk);
    HIPCHK(hipMemcpyAsync(keys, dk, n * 128, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    ctx->release(ds);
    ctx->release(dk);
    return RV_OK;
}

extern "C" int rv_hook_prg_blocks(rv_ctx* ctx, const uint8_t* keys, size_t n_keys, uint64_t first_block, size_t n_blocks,
                                  uint8_t* out) {
    if (!ctx || !keys || !out || !n_keys || !n_blocks) return RV_E_ARG;
    HIPCHK(hipSetDevice(ctx->device));
    uint8_t *dk = nullptr, *drk = nullptr, *dout = nullptr;
    int rc;
    if ((rc = dalloc(ctx, n_keys * 16, &dk)) || (rc = dalloc(ctx, n_keys * RK_BYTES, &drk)) || (rc = dalloc(ctx, n_keys * n_blocks * 16, &dout)))
        return rc;
    HIPCHK(hipMemcpyAsync(dk, keys, n_keys * 16, hipMemcpyHostToDevice, ctx->stream));
    launch_key_schedule(ctx->stream, dk, (uint32_t)n_keys, drk);
    launch_aes_blocks(ctx->stream, drk, (uint32_t)n_keys, first_block, n_blocks, dout);
    HIPCHK(hipMemcpyAsync(out, dout, n_keys * n_blocks * 16, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    ctx->release(dk);
    ctx->release(drk);
    ctx->release(dout);
    return RV_OK;
}

extern "C" int rv_hook_sharegen_gf2(rv_ctx* ctx, const uint8_t* keys, const uint32_t omit[8], size_t n, uint64_t* out) {
    if (!ctx || !keys || !omit || !out || !n) return RV_E_ARG;
    HIPCHK(hipSetDevice(ctx->device));
    const uint32_t R = 8, NQ = 2;
    uint8_t *dk = nullptr, *drk = nullptr;
    uint32_t *d_rk = nullptr, *d_keep = nullptr, *d_masks = nullptr;
    uint32_t keep[2] = {0xFFFFFFFFu, 0xFFFFFFFFu};
    for (uint32_t r = 0; r < 8; r++) {
        if (omit[r] > 8) return RV_E_ARG;
        if (omit[r] < 8) keep[r / 4] &= ~(1u << (31 - 8 * (r % 4) - omit[r]));
    }
    const uint64_t n_blocks = (n + 127) / 128;
    int rc;
    if ((rc = dalloc(ctx, (size_t)R * 128, &dk)) || (rc = dalloc(ctx, (size_t)R * 8 * RK_BYTES, &drk)) ||
        (rc = dalloc(ctx, (size_t)RK_AREAS * 128 * NQ, &d_rk)) || (rc = dalloc(ctx, NQ, &d_keep)) ||
        (rc = dalloc(ctx, (size_t)n_blocks * 128 * NQ, &d_masks)))
        return rc;
    HIPCHK(hipMemcpyAsync(dk, keys, (size_t)R * 128, hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(hipMemcpyAsync(d_keep, keep, sizeof keep, hipMemcpyHostToDevice, ctx->stream));
    launch_key_schedule(ctx->stream, dk, R * 8, drk);
    launch_bitslice_rk(ctx->stream, drk, NQ, d_rk);
    launch_aes_gf2_masks(ctx->stream, d_rk, d_keep, NQ, 0, n_blocks, d_masks);
    std::vector<uint32_t> tmp((size_t)n_blocks * 128 * NQ);
    HIPCHK(hipMemcpyAsync(tmp.data(), d_masks, tmp.size() * 4, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    for (size_t m = 0; m < n; m++) out[m] = ((uint64_t)tmp[2 * m] << 32) | tmp[2 * m + 1];
    ctx->release(dk);
    ctx->release(drk);
    ctx->release(d_rk);
    ctx->release(d_keep);
    ctx->release(d_masks);
    return RV_OK;
}

extern "C" int rv_hook_sharegen_z64(rv_ctx* ctx, const uint8_t* keys, const uint32_t omit[8], size_t n, uint64_t* out) {
    if (!ctx || !keys || !omit || !out || !n) return RV_E_ARG;
    HIPCHK(hipSetDevice(ctx->device));
    const uint32_t R = 8, NQ = 2;
    uint8_t *dk = nullptr, *drk = nullptr;
    uint32_t *d_rk = nullptr, *d_keep = nullptr;
    uint64_t* d_masks = nullptr;
    uint32_t keep[2] = {0xFFFFFFFFu, 0xFFFFFFFFu};
    for (uint32_t r = 0; r < 8; r++) {
        if (omit[r] > 8) return RV_E_ARG;
        if (omit[r] < 8) keep[r / 4] &= ~(1u << (31 - 8 * (r % 4) - omit[r]));
    }
    const uint64_t n_blocks = (n + 1) / 2;
    int rc;
    if ((rc = dalloc(ctx, (size_t)R * 128, &dk)) || (rc = dalloc(ctx, (size_t)R * 8 * RK_BYTES, &drk)) ||
        (rc = dalloc(ctx, (size_t)RK_AREAS * 128 * NQ, &d_rk)) || (rc = dalloc(ctx, NQ, &d_keep)) ||
        (rc = dalloc(ctx, (size_t)n_blocks * 2 * R * 8, &d_masks)))
        return rc;
    HIPCHK(hipMemcpyAsync(dk, keys, (size_t)R * 128, hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(hipMemcpyAsync(d_keep, keep, sizeof keep, hipMemcpyHostToDevice, ctx->stream));
    launch_key_schedule(ctx->stream, dk, R * 8, drk);
    launch_bitslice_rk(ctx->stream, drk, NQ, d_rk);
    launch_aes_z64_masks(ctx->stream, d_rk, d_keep, NQ, n_blocks, d_masks);
    HIPCHK(hipMemcpyAsync(out, d_masks, n * 64 * 8, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    ctx->release(dk);
    ctx->release(drk);
    ctx->release(d_rk);
    ctx->release(d_keep);
    ctx->release(d_masks);
    return RV_OK;
}

// Every mask generator as a shard launches it (shard.inc: shard_setup_prg), at any shard width, counter window and key setup
extern "C" int rv_hook_maskgen(rv_ctx* ctx, const uint8_t* seeds, uint32_t R, const uint8_t* omit, uint32_t generator, uint32_t key_path,
                               uint64_t first_block, uint64_t n_blocks, void* out) {
    if (!ctx || !seeds || !out || !n_blocks || generator > 2 || key_path > 1) return RV_E_ARG;
    if (!R || R % 8 || R > RV_TOTAL_REPS) return RV_E_ARG;
    if (first_block > RV_MAX_CTR_BLOCKS || n_blocks > RV_MAX_CTR_BLOCKS - first_block) return RV_E_UNSUPPORTED;
    const uint32_t NQ = R / 4;
    const bool col4 = generator == 1;
    if (col4 && !aes_col4_supports(NQ)) return RV_E_UNSUPPORTED;
    std::vector<uint32_t> keep(NQ, 0xFFFFFFFFu);
    if (omit)
        for (uint32_t r = 0; r < R; r++) {
            if (omit[r] > 8) return RV_E_ARG;
            if (omit[r] < 8) keep[r / 4] &= ~(1u << (31 - 8 * (r % 4) - omit[r]));
        }
    HIPCHK(hipSetDevice(ctx->device));
    // what the launch writes: GF(2) rows [n_blocks * 128][NQ] u32, Z64 rows [2 * n_blocks][NQ * 32] u64
    const size_t out_words = generator == 2 ? (size_t)n_blocks * 2 * NQ * 32 * 2 : (size_t)n_blocks * 128 * NQ;
    uint8_t *ds = nullptr, *dk = nullptr, *drkb = nullptr;
    uint32_t *d_rk = nullptr, *d_img = nullptr, *d_keep = nullptr, *d_out = nullptr;
    int rc;
    if ((rc = dalloc(ctx, (size_t)R * 16, &ds)) || (rc = dalloc(ctx, (size_t)R * 128, &dk)) || (rc = dalloc(ctx, (size_t)R * 8 * RK_BYTES, &drkb)) ||
        (rc = dalloc(ctx, (size_t)RK_AREAS * 128 * NQ, &d_rk)) || (omit && (rc = dalloc(ctx, NQ, &d_keep))) ||
        (col4 && (rc = dalloc(ctx, aes_col4_image_bytes(NQ) / 4, &d_img))) || (rc = dalloc(ctx, out_words, &d_out)))
        return rc;
    HIPCHK(hipMemcpyAsync(ds, seeds, (size_t)R * 16, hipMemcpyHostToDevice, ctx->stream));
    if (omit) HIPCHK(hipMemcpyAsync(d_keep, keep.data(), (size_t)NQ * 4, hipMemcpyHostToDevice, ctx->stream));
    if (key_path == 0) {
        launch_expand_seeds(ctx->stream, ds, R, dk);
        launch_key_schedule(ctx->stream, dk, R * 8, drkb);
        launch_bitslice_rk(ctx->stream, drkb, NQ, d_rk);
        if (col4) launch_rk_col4(ctx->stream, d_rk, NQ, d_img);
    } else {
        launch_setup_keys(ctx->stream, ds, NQ, dk, drkb, d_rk, d_img);
    }
    if (generator == 0)
        launch_aes_gf2_masks(ctx->stream, d_rk, d_keep, NQ, first_block, n_blocks, d_out);
    else if (generator == 1)
        launch_aes_gf2_masks_col4(ctx->stream, d_img, d_keep, NQ, first_block, n_blocks, d_out);
    else
        launch_aes_z64_masks(ctx->stream, d_rk, d_keep, NQ, n_blocks, (uint64_t*)d_out, first_block);
    HIPCHK(hipMemcpyAsync(out, d_out, out_words * 4, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    ctx->release(ds);
    ctx->release(dk);
    ctx->release(drkb);
    ctx->release(d_rk);
    if (d_keep) ctx->release(d_keep);
    if (d_img) ctx->release(d_img);
    ctx->release(d_out);
    return RV_OK;
}

extern "C" int rv_hook_blake3(rv_ctx* ctx, const uint8_t* data, size_t n_streams, size_t len, uint8_t* out) {
    if (!ctx || !out || !n_streams || (len && !data)) return RV_E_ARG;
    HIPCHK(hipSetDevice(ctx->device));
    // lay the streams out in transcript row format: row e, repetition r = stream r
    const uint32_t R = (uint32_t)((n_streams + 7) / 8 * 8), NQ = R / 4;
    std::vector<uint32_t> rows((size_t)std::max<size_t>(len, 1) * NQ, 0);
    for (size_t r = 0; r < n_streams; r++)
        for (size_t e = 0; e < len; e++) rows[e * NQ + r / 4] |= (uint32_t)data[r * len + e] << (24 - 8 * (r % 4));
    uint32_t *d_rows = nullptr, *cva = nullptr, *cvb = nullptr, *dig = nullptr;
    const size_t cvw = b3_stream_scratch_words(len, R);
    int rc;
    if ((rc = dalloc(ctx, rows.size(), &d_rows)) || (rc = dalloc(ctx, cvw, &cva)) || (rc = dalloc(ctx, cvw, &cvb)) ||
        (rc = dalloc(ctx, (size_t)R * 8, &dig)))
        return rc;
    HIPCHK(hipMemcpyAsync(d_rows, rows.data(), rows.size() * 4, hipMemcpyHostToDevice, ctx->stream));
    launch_b3_stream(ctx->stream, d_rows, len, NQ, cva, cvb, dig);
    std::vector<uint32_t> h((size_t)R * 8);
    HIPCHK(hipMemcpyAsync(h.data(), dig, h.size() * 4, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    memcpy(out, h.data(), n_streams * 32);
    ctx->release(d_rows);
    ctx->release(cva);
    ctx->release(cvb);
    ctx->release(dig);
    return RV_OK;
}

// DomainGF2::reconstruct / DomainZ64::reconstruct (gf2/domain.rs:47-63, z64/domain.rs:53-61) through the device
// functions the interpreters use (recon32 on the two quad words of a packed share; the 4-lane shuffle sum)
extern "C" int rv_hook_gf2_reconstruct(rv_ctx* ctx, const uint64_t* shares, size_t n, uint64_t* out) {
    if (!ctx || (n && (!shares || !out))) return RV_E_ARG;
    if (!n) return RV_OK;
    HIPCHK(hipSetDevice(ctx->device));
    uint64_t *d_in = nullptr, *d_out = nullptr;
    int rc;
    if ((rc = dalloc(ctx, n, &d_in)) || (rc = dalloc(ctx, n, &d_out))) return rc;
    HIPCHK(hipMemcpyAsync(d_in, shares, n * 8, hipMemcpyHostToDevice, ctx->stream));
    launch_hook_recon_gf2(ctx->stream, d_in, n, d_out);
    HIPCHK(hipMemcpyAsync(out, d_out, n * 8, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    ctx->release(d_in);
    ctx->release(d_out);
    return RV_OK;
}

extern "C" int rv_hook_z64_reconstruct(rv_ctx* ctx, const uint64_t* shares, size_t n, uint64_t* out) {
    if (!ctx || (n && (!shares || !out))) return RV_E_ARG;
    if (!n) return RV_OK;
    HIPCHK(hipSetDevice(ctx->device));
    uint64_t *d_in = nullptr, *d_out = nullptr;
    int rc;
    if ((rc = dalloc(ctx, n * 64, &d_in)) || (rc = dalloc(ctx, n * 8, &d_out))) return rc;
    HIPCHK(hipMemcpyAsync(d_in, shares, n * 64 * 8, hipMemcpyHostToDevice, ctx->stream));
    launch_hook_recon_z64(ctx->stream, d_in, n, d_out);
    HIPCHK(hipMemcpyAsync(out, d_out, n * 8 * 8, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    ctx->release(d_in);
    ctx->release(d_out);
    return RV_OK;
}

// ------------------------------------------------------------------------------------
// The opening and unpacking kernels (open.hip, z64.hip), one production launch at a time on caller-supplied data: the launch_*
// function is called unchanged, so the tile and the grid are production's.  Every output buffer arrives pre-filled, is uploaded
// before the launch and comes back whole: a byte the launch did not write keeps the caller's fill.  Whatever a kernel relies on
// its callers for (offsets inside the buffers, at most RV_ONLINE_REPS opened repetitions, an out_nq / out_r that holds every
// opened repetition) is checked here on the host, RV_E_ARG before anything is allocated or launched.
// ------------------------------------------------------------------------------------
namespace {
constexpr uint64_t HOOK_MAX = 1ull << 36;  // items / bytes: far above any test, far below where the checks' sums could wrap

// device buffers of one hook call, back in the arena on every return path
struct HookBufs {
    rv_ctx* ctx;
    std::vector<void*> owned;
    explicit HookBufs(rv_ctx* c) : ctx(c) {}
    ~HookBufs() {
        for (void* p : owned) ctx->release(p);
    }
    template <class T>
    int up(const T* src, size_t count, T** d) {  // count elements from the host (src may be NULL when count is 0)
        int rc = dalloc(ctx, std::max<size_t>(count, 1), d);
        if (rc) return rc;
        owned.push_back(*d);
        if (count) HIPCHK(hipMemcpyAsync(*d, src, count * sizeof(T), hipMemcpyHostToDevice, ctx->stream));
        return RV_OK;
    }
    template <class T>
    int filled(int byte, size_t count, T** d) {  // count elements of `byte` bytes
        int rc = dalloc(ctx, std::max<size_t>(count, 1), d);
        if (rc) return rc;
        owned.push_back(*d);
        HIPCHK(hipMemsetAsync(*d, byte, std::max<size_t>(count, 1) * sizeof(T), ctx->stream));
        return RV_OK;
    }
    template <class T>
    int down(T* dst, const T* d, size_t count) {
        if (count) HIPCHK(hipMemcpyAsync(dst, d, count * sizeof(T), hipMemcpyDeviceToHost, ctx->stream));
        return RV_OK;
    }
};

// a shard's opening map: R a multiple of 8 up to 256, values 0..8, at most RV_ONLINE_REPS below 8 (ex_slots clamps there)
bool hook_map_ok(uint32_t R, const uint8_t* omit) {
    if (!omit || !R || R % 8 || R > RV_TOTAL_REPS) return false;
    uint32_t n_on = 0;
    for (uint32_t r = 0; r < R; r++) {
        if (omit[r] > 8) return false;
        n_on += omit[r] < 8;
    }
    return n_on <= RV_ONLINE_REPS;
}
// [at[r], at[r] + len[r]) (or + fixed) inside a buffer of `bytes`, for every opened repetition
bool hook_ranges_ok(uint32_t R, const uint8_t* omit, const uint64_t* at, const uint64_t* len, uint64_t fixed, uint64_t bytes) {
    if (!at) return false;
    for (uint32_t r = 0; r < R; r++) {
        const uint64_t l = len ? len[r] : fixed;
        if (omit[r] < 8 && (at[r] > bytes || l > bytes - at[r])) return false;
    }
    return true;
}
// the OnlineList of a map as k_fs_challenge leaves it: the opened repetitions in order, each with its vector's offset
OnlineList hook_online_list(uint32_t R, const uint8_t* omit, const uint64_t* dst_off) {
    OnlineList ol{};
    for (uint32_t r = 0; r < R; r++)
        if (omit[r] < 8) {
            ol.rep[ol.n] = r;
            ol.dst[ol.n] = dst_off[r];
            ol.n++;
        }
    return ol;
}
}  // namespace

extern "C" int rv_hook_extract_bits(rv_ctx* ctx, const uint32_t* stream, uint64_t stream_rows, const uint32_t* rows, uint64_t n_items, uint32_t R, int kind,
                                    const uint8_t* omit, const uint64_t* dst_off, uint8_t* out, uint64_t out_bytes, uint8_t* out2, uint32_t n_direct,
                                    const uint64_t* gaps, uint32_t* tile) {
    if (!ctx || !out || !tile || (kind != 0 && kind != 1) || !hook_map_ok(R, omit)) return RV_E_ARG;
    if (n_items > HOOK_MAX || stream_rows > HOOK_MAX || out_bytes > HOOK_MAX || (stream_rows && !stream)) return RV_E_ARG;
    const uint64_t n_bytes = n_items / 8 + 1;
    if (!hook_ranges_ok(R, omit, dst_off, nullptr, n_bytes, out_bytes)) return RV_E_ARG;
    if (rows) {
        for (uint64_t i = 0; i < n_items; i++)
            if (rows[i] >= stream_rows) return RV_E_ARG;
    } else if (n_items > stream_rows) {
        return RV_E_ARG;
    }
    if ((n_direct || gaps) && (!out2 || kind != 0)) return RV_E_ARG;
    OpenDirect od;
    if (gaps) {
        // {first, rec, corr_at, corr_len, n_rec, rep_limit, rvec_at, with OpenDirect}: n_rec records of rec bytes from `first` inside the image,
        // each with its corrections inside it and -- for k_copy_gaps to leave words out -- its broadcast vector in front of them
        const uint64_t first = gaps[0], rec = gaps[1], corr_at = gaps[2], corr_len = gaps[3], n_rec = gaps[4], rep_limit = gaps[5], rvec_at = gaps[6];
        if (n_rec > RV_ONLINE_REPS || rep_limit > RV_TOTAL_REPS || first > out_bytes || rec > out_bytes || n_rec * rec > out_bytes - first) return RV_E_ARG;
        if (corr_at > rec || corr_len > rec - corr_at) return RV_E_ARG;
        if (gaps[7]) {
            if (rvec_at > corr_at || n_bytes > corr_at - rvec_at) return RV_E_ARG;
            od.n_direct = n_direct, od.tile = extract_tile_bytes(n_items), od.rvec_at = rvec_at, od.rvec_len = n_bytes;
        }
    }
    HIPCHK(hipSetDevice(ctx->device));
    const uint32_t NQ = R / 4;
    uint8_t omit_all[RV_TOTAL_REPS];  // (k_copy_gaps counts over the whole proof's map)
    for (uint32_t r = 0; r < RV_TOTAL_REPS; r++) omit_all[r] = r < R ? omit[r] : (uint8_t)8;
    HookBufs B(ctx);
    uint32_t *d_stream = nullptr, *d_rows = nullptr;
    uint8_t *d_omit = nullptr, *d_out = nullptr, *d_out2 = nullptr;
    uint64_t* d_dst = nullptr;
    int rc;
    if ((rc = B.up(stream, (size_t)stream_rows * NQ, &d_stream)) || (rows && (rc = B.up(rows, (size_t)n_items, &d_rows))) ||
        (rc = B.up(omit_all, (size_t)RV_TOTAL_REPS, &d_omit)) || (rc = B.up(dst_off, (size_t)R, &d_dst)) || (rc = B.up(out, (size_t)out_bytes, &d_out)) ||
        (out2 && (rc = B.up(out2, (size_t)out_bytes, &d_out2))))
        return rc;
    launch_extract_bits(ctx->stream, d_stream, d_rows, n_items, NQ, kind, d_omit, d_dst, d_out, d_out2, n_direct);
    if (gaps)
        launch_copy_gaps(ctx->stream, d_out, d_out2, out_bytes, gaps[0], gaps[1], gaps[2], gaps[3], (uint32_t)gaps[4], d_omit, (uint32_t)gaps[5], od);
    HIPCHK(hipGetLastError());
    *tile = extract_tile_bytes(n_items);
    if ((rc = B.down(out, d_out, (size_t)out_bytes)) || (out2 && (rc = B.down(out2, d_out2, (size_t)out_bytes)))) return rc;
    HIPCHK(hipStreamSynchronize(ctx->stream));
    return RV_OK;
}

extern "C" int rv_hook_extract_from_bits(rv_ctx* ctx, const uint8_t* bits, uint64_t n_items, uint32_t R, const uint8_t* omit, const uint64_t* dst_off,
                                         uint32_t rep_min, uint8_t* out, uint64_t out_bytes, uint32_t* tile) {
    if (!ctx || !out || !tile || !hook_map_ok(R, omit) || n_items > HOOK_MAX || out_bytes > HOOK_MAX || (n_items && !bits)) return RV_E_ARG;
    if (!hook_ranges_ok(R, omit, dst_off, nullptr, n_items / 8 + 1, out_bytes)) return RV_E_ARG;
    HIPCHK(hipSetDevice(ctx->device));
    const OnlineList ol = hook_online_list(R, omit, dst_off);
    HookBufs B(ctx);
    uint8_t *d_bits = nullptr, *d_out = nullptr;
    OnlineList* d_ol = nullptr;
    int rc;
    if ((rc = B.up(bits, (size_t)n_items * (R / 8), &d_bits)) || (rc = B.up(&ol, 1, &d_ol)) || (rc = B.up(out, (size_t)out_bytes, &d_out))) return rc;
    launch_extract_from_bits(ctx->stream, d_bits, n_items, R / 4, d_ol, d_out, rep_min);
    HIPCHK(hipGetLastError());
    *tile = extract_from_bits_tile_bytes(n_items);
    if ((rc = B.down(out, d_out, (size_t)out_bytes))) return rc;
    HIPCHK(hipStreamSynchronize(ctx->stream));
    return RV_OK;
}

extern "C" int rv_hook_pack_corr_all(rv_ctx* ctx, const uint8_t* bits, uint64_t n_items, uint64_t byte0, uint64_t n_bytes, uint64_t pitch, uint8_t* out) {
    if (!ctx || !out || n_items > HOOK_MAX || byte0 > HOOK_MAX || (n_items && !bits)) return RV_E_ARG;
    if (!pitch || pitch % 128 || pitch > (1ull << 24) || n_bytes > pitch) return RV_E_ARG;  // (the kernel writes whole 16-byte words: up to the pitch's padding)
    HIPCHK(hipSetDevice(ctx->device));
    HookBufs B(ctx);
    uint8_t *d_bits = nullptr, *d_out = nullptr;
    int rc;
    if ((rc = B.up(bits, (size_t)n_items * 32, &d_bits)) || (rc = B.up(out, (size_t)RV_TOTAL_REPS * pitch, &d_out))) return rc;
    launch_pack_corr_all(ctx->stream, d_bits, n_items, byte0, n_bytes, pitch, d_out);
    HIPCHK(hipGetLastError());
    if ((rc = B.down(out, d_out, (size_t)RV_TOTAL_REPS * pitch))) return rc;
    HIPCHK(hipStreamSynchronize(ctx->stream));
    return RV_OK;
}

extern "C" int rv_hook_unpack_bits(rv_ctx* ctx, const uint8_t* blob, uint64_t blob_bytes, const uint64_t* src_off, const uint64_t* src_len, const uint8_t* omit,
                                   uint64_t n_items, uint32_t R, int kind, uint32_t out_nq, uint64_t first_item, uint32_t* rows_out) {
    if (!ctx || !rows_out || (kind != 0 && kind != 1) || !hook_map_ok(R, omit) || !src_len) return RV_E_ARG;
    if (n_items > HOOK_MAX || first_item > HOOK_MAX || blob_bytes > HOOK_MAX || (blob_bytes && !blob)) return RV_E_ARG;
    if (!hook_ranges_ok(R, omit, src_off, src_len, 0, blob_bytes)) return RV_E_ARG;
    // supplied_nq (verify.inc): full rows, or sixteen quad words when no repetition beyond them is opened
    const uint32_t NQ = R / 4;
    if (out_nq != NQ) {
        if (out_nq != 16 || NQ < 16) return RV_E_ARG;
        for (uint32_t r = 64; r < R; r++)
            if (omit[r] < 8) return RV_E_ARG;
    }
    HIPCHK(hipSetDevice(ctx->device));
    HookBufs B(ctx);
    uint8_t *d_blob = nullptr, *d_omit = nullptr;
    uint64_t *d_off = nullptr, *d_len = nullptr;
    uint32_t* d_rows = nullptr;
    const size_t n_words = (size_t)n_items * out_nq;
    int rc;
    if ((rc = B.up(blob, (size_t)blob_bytes, &d_blob)) || (rc = B.up(src_off, (size_t)R, &d_off)) || (rc = B.up(src_len, (size_t)R, &d_len)) ||
        (rc = B.up(omit, (size_t)R, &d_omit)) || (rc = B.up(rows_out, n_words, &d_rows)))
        return rc;
    launch_unpack_bits(ctx->stream, d_blob, d_off, d_len, d_omit, n_items, NQ, kind, d_rows, out_nq, first_item);
    HIPCHK(hipGetLastError());
    if ((rc = B.down(rows_out, d_rows, n_words))) return rc;
    HIPCHK(hipStreamSynchronize(ctx->stream));
    return RV_OK;
}

extern "C" int rv_hook_extract64(rv_ctx* ctx, const uint64_t* stream, uint64_t stride_words, const uint64_t* offs, uint64_t n_items, int add_omit, uint32_t R,
                                 const uint8_t* omit, const uint64_t* dst_off, int use_list, uint32_t rep_min, uint8_t* out, uint64_t out_bytes) {
    if (!ctx || !out || !hook_map_ok(R, omit) || n_items > HOOK_MAX || stride_words > HOOK_MAX || out_bytes > HOOK_MAX || (stride_words && !stream)) return RV_E_ARG;
    if (!hook_ranges_ok(R, omit, dst_off, nullptr, 8 * n_items, out_bytes)) return RV_E_ARG;
    if (n_items) {
        uint64_t top = n_items - 1;  // the last word of a repetition's stream that is read
        if (offs) {
            top = 0;
            for (uint64_t i = 0; i < n_items; i++) top = std::max(top, offs[i]);
        }
        if (top > HOOK_MAX) return RV_E_ARG;
        uint64_t om_max = 0;
        for (uint32_t r = 0; r < R; r++)
            if (omit[r] < 8) om_max = std::max<uint64_t>(om_max, omit[r]);
        if (top + (add_omit ? om_max : 0) >= stride_words) return RV_E_ARG;
    }
    HIPCHK(hipSetDevice(ctx->device));
    const OnlineList ol = hook_online_list(R, omit, dst_off);
    HookBufs B(ctx);
    uint64_t *d_stream = nullptr, *d_offs = nullptr, *d_dst = nullptr;
    uint8_t *d_omit = nullptr, *d_out = nullptr;
    OnlineList* d_ol = nullptr;
    int rc;
    if ((rc = B.up(stream, (size_t)R * stride_words, &d_stream)) || (offs && (rc = B.up(offs, (size_t)n_items, &d_offs))) || (rc = B.up(omit, (size_t)R, &d_omit)) ||
        (rc = B.up(dst_off, (size_t)R, &d_dst)) || (use_list && (rc = B.up(&ol, 1, &d_ol))) || (rc = B.up(out, (size_t)out_bytes, &d_out)))
        return rc;
    launch_extract64(ctx->stream, d_stream, stride_words, d_offs, n_items, add_omit ? 1 : 0, R, d_omit, d_dst, d_out, d_ol, rep_min);
    HIPCHK(hipGetLastError());
    if ((rc = B.down(out, d_out, (size_t)out_bytes))) return rc;
    HIPCHK(hipStreamSynchronize(ctx->stream));
    return RV_OK;
}

extern "C" int rv_hook_unpack64(rv_ctx* ctx, const uint8_t* blob, uint64_t blob_bytes, const uint64_t* src_off, const uint64_t* src_len, const uint8_t* omit,
                                uint64_t n_items, uint32_t R, uint32_t out_r, uint64_t* out) {
    if (!ctx || !out || !hook_map_ok(R, omit) || !src_len || n_items > HOOK_MAX || blob_bytes > HOOK_MAX || (blob_bytes && !blob)) return RV_E_ARG;
    if (!hook_ranges_ok(R, omit, src_off, src_len, 0, blob_bytes)) return RV_E_ARG;
    // supplied_r64 (verify.inc): every repetition, or the first 64 when no other is opened
    if (out_r != R) {
        if (out_r != 64 || R < 64) return RV_E_ARG;
        for (uint32_t r = 64; r < R; r++)
            if (omit[r] < 8) return RV_E_ARG;
    }
    HIPCHK(hipSetDevice(ctx->device));
    HookBufs B(ctx);
    uint8_t *d_blob = nullptr, *d_omit = nullptr;
    uint64_t *d_off = nullptr, *d_len = nullptr, *d_out = nullptr;
    const size_t n_words = (size_t)n_items * out_r;
    int rc;
    if ((rc = B.up(blob, (size_t)blob_bytes, &d_blob)) || (rc = B.up(src_off, (size_t)R, &d_off)) || (rc = B.up(src_len, (size_t)R, &d_len)) ||
        (rc = B.up(omit, (size_t)R, &d_omit)) || (rc = B.up(out, n_words, &d_out)))
        return rc;
    launch_unpack64(ctx->stream, d_blob, d_off, d_len, d_omit, n_items, R, d_out, out_r);
    HIPCHK(hipGetLastError());
    if ((rc = B.down(out, d_out, n_words))) return rc;
    HIPCHK(hipStreamSynchronize(ctx->stream));
    return RV_OK;
}

// ------------------------------------------------------------------------------------
// Which executor runs which level (interp.hip, ldsrun.hip): the compiled level table with the narrow-run plan, and the counters of the
// launches issued.  Ten int32 per level: lo, mul11, mul, xor2, xork, hi (LevelRange), 1 when the level holds Z64 gates, the index of
// its narrow run and that run's `tiny` (-1, -1: none), the index of its LDS run (-1: none; always -1 without a circuit).
// ------------------------------------------------------------------------------------
static void hook_write_levels(const Compiled& cc, const std::vector<rv_circuit::NarrowRun>& runs, const std::vector<int32_t>& run_of_level,
                              const std::vector<int32_t>* lds_run_of_level, int32_t* out, size_t cap, size_t* n_levels) {
    const size_t n = cc.level_start.empty() ? 0 : cc.level_start.size() - 1;
    *n_levels = n;
    for (size_t l = 0; l < n && l < cap; l++) {
        const LevelRange& r = cc.level_range[l];
        int32_t* o = out + 10 * l;
        o[0] = (int32_t)r.lo, o[1] = (int32_t)r.mul11, o[2] = (int32_t)r.mul, o[3] = (int32_t)r.xor2, o[4] = (int32_t)r.xork, o[5] = (int32_t)r.hi;
        o[6] = !cc.level_start64.empty() && cc.level_start64[l + 1] > cc.level_start64[l];
        o[7] = run_of_level[l];
        o[8] = run_of_level[l] >= 0 ? runs[(size_t)run_of_level[l]].tiny : -1;
        o[9] = lds_run_of_level ? (*lds_run_of_level)[l] : -1;
    }
}

extern "C" int rv_hook_compile_levels(const rv_op* ops, size_t n_ops, size_t z64_wires, size_t gf2_wires, uint32_t flags, int32_t* out, size_t cap,
                                      size_t* n_levels) {
    if (!n_levels || (cap && !out) || (n_ops && !ops) || (flags & ~RV_COMPILE_WHOLE_PROVER)) return RV_E_ARG;
    try {
        Compiled cc;
        const int rc = compile_ops(ops, n_ops, z64_wires, gf2_wires, cc, nullptr, ((flags & RV_COMPILE_WHOLE_PROVER) && !getenv("RV_LAZY_K")) ? RV_LIN_K : 0);
        if (rc) return rc;
        std::vector<rv_circuit::NarrowRun> runs;
        std::vector<int32_t> run_of_level;
        plan_narrow_runs(cc, runs, run_of_level);
        hook_write_levels(cc, runs, run_of_level, nullptr, out, cap, n_levels);
        return RV_OK;
    } catch (...) {
        g_last_error = "out of host memory";
        return RV_E_NOMEM;
    }
}

extern "C" int rv_hook_circuit_levels(const rv_circuit* c, int32_t* out, size_t cap, size_t* n_levels, int* vclr_ok, int* general_levels) {
    if (!c || !n_levels || (cap && !out)) return RV_E_ARG;
    hook_write_levels(c->cc, c->narrow_runs, c->run_of_level, &c->lds_run_of_level, out, cap, n_levels);
    if (vclr_ok) *vclr_ok = c->vclr_ok;
    if (general_levels) *general_levels = c->general_levels;
    return RV_OK;
}

extern "C" int rv_hook_interp_launches(uint64_t counts[][4], int reset) {
    if (!counts) return RV_E_ARG;
    interp_launch_counts(counts, reset != 0);
    return RV_OK;
}

// ------------------------------------------------------------------------------------
// Which executor runs a Z64 level (aes.hip: k_z64_fused, z64.hip: k_interp64 / k_interp64_b): the launch counters, the fused
// launcher's grid arithmetic and the fused level table of a program with the reason a circuit is not eligible.
// ------------------------------------------------------------------------------------
extern "C" int rv_hook_interp64_launches(uint64_t counts[][2], int reset) {
    if (!counts) return RV_E_ARG;
    interp64_launch_counts(counts, reset != 0);
    return RV_OK;
}

extern "C" int rv_hook_z64_fused_grid(uint32_t qw, uint32_t n_qg, uint32_t cus, uint32_t n_mul, uint32_t n_lin, uint32_t n_oth, uint32_t out[5]) {
    if (!out || (qw != 16 && qw != 8)) return RV_E_ARG;
    const Z64FGrid g = z64_fused_grid(qw, n_qg, cus ? cus : z64_fused_cus(), n_mul, n_lin, n_oth);
    out[0] = g.chunks, out[1] = g.mul_per, out[2] = g.lin_per, out[3] = g.oth_per, out[4] = g.lin_bias;
    return RV_OK;
}

extern "C" int rv_hook_z64_fused_levels(const rv_op* ops, size_t n_ops, size_t z64_wires, size_t gf2_wires, uint32_t flags, uint32_t* out, size_t cap,
                                        size_t* n_levels, int* eligible) {
    if (!n_levels || !eligible || (cap && !out) || (n_ops && !ops) || (flags & ~RV_COMPILE_WHOLE_PROVER)) return RV_E_ARG;
    try {
        Compiled cc;
        const int rc = compile_ops(ops, n_ops, z64_wires, gf2_wires, cc, nullptr, ((flags & RV_COMPILE_WHOLE_PROVER) && !getenv("RV_LAZY_K")) ? RV_LIN_K : 0);
        if (rc) return rc;
        std::vector<Gate64> sorted;
        std::vector<Z64FLevel> levels;
        std::vector<std::pair<uint64_t, uint64_t>> runs;
        int why = Z64F_NONE;
        build_z64_fused(cc, sorted, levels, runs, &why, true);
        *eligible = why;
        *n_levels = levels.size();
        for (size_t l = 0; l < levels.size() && l < cap; l++) {
            uint32_t* o = out + 4 * l;
            o[0] = levels[l].mul0, o[1] = levels[l].mul1, o[2] = levels[l].lin1, o[3] = levels[l].oth1;
        }
        return RV_OK;
    } catch (...) {
        g_last_error = "out of host memory";
        return RV_E_NOMEM;
    }
}
