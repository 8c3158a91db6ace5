// The body of one Z64 dependency level for one proof (gates [lo, hi) of `gates`, parameter block `p`), textually shared by
// k_interp64 and k_interp64_b (z64.hip): included, not called, so that the single-proof kernel compiles to exactly the code it
// had before the batched one existed (an inlined device function changes its register allocation).
    const uint32_t S = p.R * 8;   // u64 per row
    const uint32_t S2 = p.R * 4;  // lanes per gate
    const uint32_t tid = blockIdx.x * blockDim.x + threadIdx.x;
    const uint32_t l = tid % S2;
    const uint32_t r = l >> 2, pk = l & 3;  // this lane holds players 2*pk and 2*pk + 1 of repetition r
    const uint32_t worker = tid / S2, n_workers = (gridDim.x * blockDim.x) / S2;
    const uint32_t om = (MODE == MODE_VERIFY) ? p.omit[r] : 8u;
    const bool online = om < 8;  // online-verified repetition (MODE_VERIFY only)
    const bool mine = (om >> 1) == pk;  // the omitted player sits in this lane (slot om & 1)
    for (uint32_t gi = lo + worker; gi < hi; gi += n_workers) {
        const Gate64 g = gates[gi];
        uint64_t* dm = p.wmask + (size_t)g.dst * S + 2 * l;
        uint64_t* dc = p.wcorr + (size_t)g.dst * p.R + r;
        // an operand's mask row: its own wmask row, or the fresh PRG mask row that IS the wire's mask (Input / Random / Mul results)
        const uint64_t* am = ((g.am & G64_MASK_ROW) ? p.masks + (size_t)(g.am & ~G64_MASK_ROW) * S : p.wmask + (size_t)g.am * S) + 2 * l;
        const uint64_t* ac = p.wcorr + (size_t)g.a * p.R + r;
        const uint64_t* bm = ((g.bm & G64_MASK_ROW) ? p.masks + (size_t)(g.bm & ~G64_MASK_ROW) * S : p.wmask + (size_t)g.bm * S) + 2 * l;
        const uint64_t* bc = p.wcorr + (size_t)g.b * p.R + r;
        switch (g.op) {
        case G64_INPUT: {
            const U2 lam = ld2(p.masks + (size_t)g.m * S + 2 * l);
            uint64_t corr;
            if (MODE == MODE_PROVE)
                corr = p.wit[g.x] - sum8(lam);
            else
                corr = online ? p.sup_in[(size_t)g.x * p.sup_r + r] : 0;
            if (pk == 0) {
                *dc = corr;
                p.on[(size_t)r * p.on_words + g.eo] = corr;
            }
            break;
        }
        case G64_ADD: {
            const U2 x = ld2(am), y = ld2(bm);
            st2(dm, U2{x.x + y.x, x.y + y.y});
            if (pk == 0) *dc = *ac + *bc;
            break;
        }
        case G64_SUB: {
            const U2 x = ld2(am), y = ld2(bm);
            st2(dm, U2{x.x - y.x, x.y - y.y});
            if (pk == 0) *dc = *ac - *bc;
            break;
        }
        case G64_ADDC:
            st2(dm, ld2(am));
            if (pk == 0) *dc = *ac + g.imm;
            break;
        case G64_SUBC:
            st2(dm, ld2(am));
            if (pk == 0) *dc = *ac - g.imm;
            break;
        case G64_MULC: {
            const U2 x = ld2(am);
            st2(dm, U2{x.x * g.imm, x.y * g.imm});
            if (pk == 0) *dc = *ac * g.imm;
            break;
        }
        case G64_CONST:
            st2(dm, U2{0, 0});
            if (pk == 0) *dc = g.imm;
            break;
        case G64_RANDOM:
            if (pk == 0) *dc = 0;
            break;
        case G64_MUL: {
            const U2 lx = ld2(am), ly = ld2(bm);
            const U2 lab = ld2(p.masks + (size_t)g.m * S + 2 * l), lnew = ld2(p.masks + (size_t)(g.m + 1) * S + 2 * l);
            const uint64_t cx = *ac, cy = *bc;
            const uint64_t a = sum8(lx), b = sum8(ly), c = sum8(lab);
            uint64_t delta = a * b - c;
            U2 s{ly.x * cx + lx.x * cy + lab.x - lnew.x, ly.y * cx + lx.y * cy + lab.y - lnew.y};
            if (MODE == MODE_VERIFY && online) {
                delta = p.sup_corr[(size_t)g.xc * p.sup_r + r];
                if (mine) {
                    const uint64_t sup = p.sup_rec[(size_t)g.x * p.sup_r + r];
                    if (om & 1) s.y += sup; else s.x += sup;
                }
            }
            st2_unaligned(p.on + (size_t)r * p.on_words + g.eo + 2 * pk, s);
            uint64_t rec = sum8(s);
            if (MODE == MODE_VERIFY && !online) rec = 0;
            if (pk == 0) {
                p.pre[(size_t)r * p.pre_words + g.ep] = delta;
                *dc = rec + delta + cx * cy;
            }
            break;
        }
        case G64_ASSERT: {
            U2 m = ld2(am);
            if (MODE == MODE_VERIFY && online && mine) {
                const uint64_t sup = p.sup_rec[(size_t)g.x * p.sup_r + r];
                if (om & 1) m.y += sup; else m.x += sup;
            }
            st2_unaligned(p.on + (size_t)r * p.on_words + g.eo + 2 * pk, m);
            {
                const uint64_t v = sum8(m) + *ac;
                if (MODE == MODE_PROVE) {
                    if (v != 0 && pk == 0) atomicOr(p.err, RV_E_WITNESS_INVALID);
                } else if (online && v != 0 && pk == 0) {
                    atomicOr(p.err, RV_DEV_ZERO_CHECK);  // online.rs:175-177 (read by RV_VERIFY_STRICT only)
                }
            }
            break;
        }
        case G64_B2A: {
            // random 64-bit value shared bitwise in GF(2): bit k = recon(fresh gf2 mask m2+k)
            const uint32_t qw = r >> 2, sh = 24 - 8 * (r & 3);
            uint64_t zval = 0, zrec = 0;
            for (int k = 0; k < 64; k++) {
                const uint32_t w = recon32_(p.masks2[(size_t)(g.m2 + k) * p.NQ + qw]);
                zval |= (uint64_t)((w >> sh) & 1u) << k;
                // revealed sum bit k: bit-per-rep corr row of the k-th G_RECON output
                const uint32_t v = p.corr2[(size_t)(g.a + k) * (p.NQ >> 1) + (qw >> 1)];
                zrec |= (uint64_t)((v >> (4 * (qw & 1) + 3 - (r & 3))) & 1u) << k;
            }
            const U2 mu = ld2(p.masks + (size_t)g.m * S + 2 * l);
            uint64_t kappa = zval - sum8(mu);
            if (MODE == MODE_VERIFY && online) kappa = p.sup_corr[(size_t)g.xc * p.sup_r + r];
            st2(dm, U2{0 - mu.x, 0 - mu.y});
            if (pk == 0) {
                p.pre[(size_t)r * p.pre_words + g.ep] = kappa;
                *dc = zrec - kappa;
            }
            break;
        }
        default:
            break;
        }
    }
