// Part of api.hip (#included there, one translation unit): the fused Z64 level kernel (aes.hip: k_z64_fused), one production
// launch per level on caller-supplied records and buffers (tests/test_gpu_z64_fused_level.py, reference tests/z64f_ref.py).

// ------------------------------------------------------------------------------------
// rv_hook_z64_fused_gates (host only): what build_z64_fused makes of an op list -- the records as the upload path sends them to
// the device, the level table, the cipher block runs of the Input rows and the eligibility code -- plus the sizes a caller needs to
// lay the buffers out.  Count, then fill: every count is returned, every array takes its first `cap` entries.
// ------------------------------------------------------------------------------------
static_assert(sizeof(Gate64) == 64, "rv_hook_z64_fused_gates / rv_hook_z64_fused_run exchange Gate64 records of 64 bytes");

extern "C" int rv_hook_z64_fused_gates(const rv_op* ops, size_t n_ops, size_t z64_wires, size_t gf2_wires, uint32_t flags, void* gates, size_t gates_cap,
                                       size_t* n_gates, uint32_t* levels, size_t levels_cap, size_t* n_levels, uint64_t* runs, size_t runs_cap,
                                       size_t* n_runs, int* eligible, uint64_t sizes[7]) {
    if (!n_gates || !n_levels || !n_runs || !eligible || (gates_cap && !gates) || (levels_cap && !levels) || (runs_cap && !runs) || (n_ops && !ops) ||
        (flags & ~RV_COMPILE_WHOLE_PROVER))
        return RV_E_ARG;
    try {
        Compiled cc;
        const int rc = compile_ops(ops, n_ops, z64_wires, gf2_wires, cc, nullptr, ((flags & RV_COMPILE_WHOLE_PROVER) && !getenv("RV_LAZY_K")) ? RV_LIN_K : 0);
        if (rc) return rc;
        std::vector<Gate64> sorted;
        std::vector<Z64FLevel> lv;
        std::vector<std::pair<uint64_t, uint64_t>> rn;
        int why = Z64F_NONE;
        build_z64_fused(cc, sorted, lv, rn, &why, true);
        *eligible = why;
        *n_gates = sorted.size();
        *n_levels = lv.size();
        *n_runs = rn.size();
        if (sorted.size() && gates_cap) memcpy(gates, sorted.data(), std::min(sorted.size(), gates_cap) * sizeof(Gate64));
        for (size_t l = 0; l < lv.size() && l < levels_cap; l++) {
            uint32_t* o = levels + 4 * l;
            o[0] = lv[l].mul0, o[1] = lv[l].mul1, o[2] = lv[l].lin1, o[3] = lv[l].oth1;
        }
        for (size_t i = 0; i < rn.size() && i < runs_cap; i++) runs[2 * i] = rn[i].first, runs[2 * i + 1] = rn[i].second;
        if (sizes) {
            sizes[0] = cc.n_ssa64, sizes[1] = cc.n_masks64, sizes[2] = cc.on_words64, sizes[3] = cc.pre_words64;
            sizes[4] = cc.n_in64, sizes[5] = cc.n_corr64, sizes[6] = cc.n_rec64;
        }
        return RV_OK;
    } catch (...) {
        g_last_error = "out of host memory";
        return RV_E_NOMEM;
    }
}

// ------------------------------------------------------------------------------------
// rv_hook_z64_fused_run: launch_z64_fused as it stands, once per level of the caller's table, in order on the context's stream, over
// quad groups [qg0, qg0 + qgn), from counter first_block.  Key setup and the Input rows' generator launches are production's
// (rv_hook_maskgen, shard.inc: shard_setup_prg); the keep words follow the shard's bit rule (verify.inc: a.keep64).  Every buffer is
// uploaded as the caller filled it and comes back whole.  What the kernel relies on its callers for is checked here on the host,
// before anything is allocated, launched or written.
// ------------------------------------------------------------------------------------
namespace {
bool z64f_row_ok(uint32_t ref, uint64_t n_ssa, uint64_t n_mask_rows) {
    return (ref & G64_MASK_ROW) ? (ref & ~G64_MASK_ROW) < n_mask_rows : ref < n_ssa;
}
// RV_OK, RV_E_ARG (a record the kernel would follow out of a buffer or does not take) or RV_E_UNSUPPORTED (a counter past the last)
int z64f_check(const rv_hook_z64f_run_args& a, const Gate64* g, bool verify) {
    int past = 0;
    for (size_t l = 0; l < a.n_levels; l++) {
        const uint32_t* lv = a.levels + 4 * l;
        if (!(lv[0] <= lv[1] && lv[1] <= lv[2] && lv[2] <= lv[3] && lv[3] <= a.n_gates)) return RV_E_ARG;
        for (uint32_t i = lv[0]; i < lv[3]; i++) {
            const Gate64& r = g[i];
            const bool two = r.op == G64_ADD || r.op == G64_SUB || r.op == G64_MUL;
            switch (r.op) {
            case G64_MUL:
                if (i >= lv[1] || (r.m & 1) || (uint64_t)r.m + 1 >= a.n_mask_rows || r.dst >= a.n_ssa) return RV_E_ARG;
                if (r.eo > a.on_words || a.on_words - r.eo < 8 || r.ep >= a.pre_words) return RV_E_ARG;
                if (verify && (r.x >= a.n_rec || r.xc >= a.n_corr)) return RV_E_ARG;
                if (a.first_block + (r.m >> 1) >= RV_MAX_CTR_BLOCKS) past = 1;
                break;
            case G64_ADD: case G64_SUB: case G64_ADDC: case G64_SUBC: case G64_MULC:
                if (i < lv[1] || i >= lv[2] || r.dst >= a.n_ssa) return RV_E_ARG;
                break;
            case G64_INPUT:
                if (i < lv[2] || r.m >= a.n_mask_rows || r.dst >= a.n_ssa || r.eo >= a.on_words || r.x >= (verify ? a.n_in : a.n_wit)) return RV_E_ARG;
                break;
            case G64_ASSERT:
                if (i < lv[2] || r.eo > a.on_words || a.on_words - r.eo < 8 || (verify && r.x >= a.n_rec)) return RV_E_ARG;
                break;
            case G64_CONST:
                if (i < lv[2] || r.dst >= a.n_ssa) return RV_E_ARG;
                break;
            default:  // Random, B2A: values that differ between repetitions
                return RV_E_ARG;
            }
            if (r.op != G64_INPUT && r.op != G64_CONST && (r.a >= a.n_ssa || !z64f_row_ok(r.am, a.n_ssa, a.n_mask_rows))) return RV_E_ARG;
            if (two && (r.b >= a.n_ssa || !z64f_row_ok(r.bm, a.n_ssa, a.n_mask_rows))) return RV_E_ARG;
        }
    }
    for (size_t i = 0; i < a.n_runs; i++) {
        const uint64_t first = a.runs[2 * i], n = a.runs[2 * i + 1];
        if (!n || first > a.n_mask_rows || n > a.n_mask_rows || 2 * (first + n) > a.n_mask_rows) return RV_E_ARG;
        if (a.first_block + first + n > RV_MAX_CTR_BLOCKS) past = 1;
    }
    return past ? RV_E_UNSUPPORTED : RV_OK;
}
}  // namespace

extern "C" int rv_hook_z64_fused_run(rv_ctx* ctx, const rv_hook_z64f_run_args* args) {
    if (!ctx || !args) return RV_E_ARG;
    const rv_hook_z64f_run_args& a = *args;
    const uint32_t R = a.R, NQ = R / 4;
    const bool verify = a.omit != nullptr;
    if (!a.seeds || !R || R % 4 || R > RV_TOTAL_REPS || a.key_path > 1) return RV_E_ARG;
    const uint32_t qw = z64_fused_qw(NQ);
    if (!qw || a.qg0 > NQ / qw || a.qgn > NQ / qw - a.qg0) return RV_E_ARG;
    if (a.n_gates >= (1ull << 32) || a.n_levels >= (1ull << 32) || a.n_ssa >= (1ull << 31) || a.n_mask_rows >= (1ull << 31) || a.on_words > HOOK_MAX ||
        a.pre_words > HOOK_MAX || a.first_block > RV_MAX_CTR_BLOCKS)
        return RV_E_ARG;
    if ((a.n_gates && !a.gates) || (a.n_levels && !a.levels) || (a.n_runs && !a.runs) || !a.wmask || !a.masks || !a.on || !a.pre || !a.err || !a.n_ssa)
        return RV_E_ARG;
    if (verify ? (!a.wcorr || !a.sup_in || !a.sup_corr || !a.sup_rec) : (!a.v || (a.n_wit && !a.wit))) return RV_E_ARG;
    std::vector<uint32_t> keep(NQ, 0xFFFFFFFFu);
    if (verify)
        for (uint32_t r = 0; r < R; r++) {
            if (a.omit[r] > 8 || (a.omit[r] < 8 && r >= a.sup_r)) return RV_E_ARG;
            if (a.omit[r] < 8) keep[r / 4] &= ~(1u << (31 - 8 * (r % 4) - a.omit[r]));
        }
    const Gate64* g = (const Gate64*)a.gates;
    if (const int rc = z64f_check(a, g, verify)) return rc;

    HIPCHK(hipSetDevice(ctx->device));
    HookBufs hb(ctx);
    const size_t S = (size_t)R * 8;
    uint8_t *ds = nullptr, *dk = nullptr, *drkb = nullptr, *d_omit = nullptr;
    uint32_t *d_rk = nullptr, *d_keep = nullptr;
    Gate64* d_gates = nullptr;
    uint64_t *d_wmask = nullptr, *d_masks = nullptr, *d_on = nullptr, *d_pre = nullptr, *d_wit = nullptr, *d_v = nullptr, *d_wcorr = nullptr, *d_in = nullptr,
             *d_corr = nullptr, *d_rec = nullptr;
    int* d_err = nullptr;
    int rc;
    if ((rc = hb.up(a.seeds, (size_t)R * 16, &ds)) || (rc = hb.filled(0, (size_t)R * 128, &dk)) || (rc = hb.filled(0, (size_t)R * 8 * RK_BYTES, &drkb)) ||
        (rc = hb.filled(0, (size_t)RK_AREAS * 128 * NQ, &d_rk)) || (rc = hb.up(g, a.n_gates, &d_gates)) || (rc = hb.up(a.wmask, a.n_ssa * S, &d_wmask)) ||
        (rc = hb.up(a.masks, a.n_mask_rows * S, &d_masks)) || (rc = hb.up(a.on, (size_t)R * a.on_words, &d_on)) ||
        (rc = hb.up(a.pre, (size_t)R * a.pre_words, &d_pre)) || (rc = hb.up(a.err, 1, &d_err)))
        return rc;
    if (verify) {
        if ((rc = hb.up(a.omit, R, &d_omit)) || (rc = hb.up(keep.data(), NQ, &d_keep)) || (rc = hb.up(a.wcorr, a.n_ssa * R, &d_wcorr)) ||
            (rc = hb.up(a.sup_in, a.n_in * a.sup_r, &d_in)) || (rc = hb.up(a.sup_corr, a.n_corr * a.sup_r, &d_corr)) ||
            (rc = hb.up(a.sup_rec, a.n_rec * a.sup_r, &d_rec)))
            return rc;
    } else {
        if ((rc = hb.up(a.wit, a.n_wit, &d_wit)) || (rc = hb.up(a.v, a.n_ssa, &d_v))) return rc;
    }
    if (a.key_path == 0) {
        launch_expand_seeds(ctx->stream, ds, R, dk);
        launch_key_schedule(ctx->stream, dk, R * 8, drkb);
        launch_bitslice_rk(ctx->stream, drkb, NQ, d_rk);
    } else {
        launch_setup_keys(ctx->stream, ds, NQ, dk, drkb, d_rk, nullptr);
    }
    // only the Input gates' rows (shard_setup_prg): a Mul's two masks come out of the level launches
    for (size_t i = 0; i < a.n_runs; i++)
        launch_aes_z64_masks(ctx->stream, d_rk, d_keep, NQ, a.runs[2 * i + 1], d_masks + (size_t)a.runs[2 * i] * 2 * S, a.first_block + a.runs[2 * i]);
    Z64FParams zp{};  // (shard.inc: fused_params)
    zp.rk = d_rk;
    zp.NQ = NQ;
    zp.wmask = d_wmask;
    zp.masks = d_masks;
    zp.on = d_on;
    zp.pre = d_pre;
    zp.on_words = a.on_words;
    zp.pre_words = a.pre_words;
    zp.wit = d_wit;
    zp.v = d_v;
    zp.err = d_err;
    zp.first_block = a.first_block;
    zp.qg0 = a.qg0;
    zp.qgn = a.qgn;
    if (verify) {
        zp.omit = d_omit;
        zp.keep = d_keep;
        zp.wcorr = d_wcorr;
        zp.sup_in = d_in;
        zp.sup_corr = d_corr;
        zp.sup_rec = d_rec;
        zp.sup_r = a.sup_r;
    }
    for (size_t l = 0; l < a.n_levels; l++) {
        const uint32_t* lv = a.levels + 4 * l;
        launch_z64_fused(ctx->stream, d_gates, Z64FLevel{lv[0], lv[1], lv[2], lv[3]}, zp);
    }
    HIPCHK(hipGetLastError());
    hb.down(a.wmask, d_wmask, a.n_ssa * S);
    hb.down(a.masks, d_masks, a.n_mask_rows * S);
    hb.down(a.on, d_on, (size_t)R * a.on_words);
    hb.down(a.pre, d_pre, (size_t)R * a.pre_words);
    hb.down(a.err, d_err, 1);
    if (verify)
        hb.down(a.wcorr, d_wcorr, a.n_ssa * R);
    else
        hb.down(a.v, d_v, a.n_ssa);
    HIPCHK(hipStreamSynchronize(ctx->stream));
    return RV_OK;
}
