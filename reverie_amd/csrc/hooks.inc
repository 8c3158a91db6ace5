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
