// The body of k_aes_z64_masks<QW>, textually shared with its recordable form B_k_aes_z64_masks<QW> (aes.hip): included, not
// called, so that the named kernel compiles to exactly its former code (inlined into it, the same body as a device function
// takes more registers and spills at QW = 8)
    __shared__ uint32_t lds_rk[11 * 128 * QW];
    constexpr uint32_t JW = 64 / QW;
    const uint32_t n_qg = NQ / QW;
    const uint32_t qg = blockIdx.x % n_qg;
    const uint64_t chunk = blockIdx.x / n_qg;
    stage_round_keys<QW>(rk, NQ, qg, lds_rk);
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint32_t ql = lane % QW, jsub = lane / QW;
    const uint32_t q = qg * QW + ql;
    const uint32_t kp = keep ? keep[q] : 0xFFFFFFFFu;
    const uint32_t* rkl = lds_rk + ql;
    const uint64_t S = (uint64_t)NQ * 32;
    const uint64_t j_lo = chunk * blocks_per_wg;
    const uint64_t j_hi = (j_lo + blocks_per_wg < n_blocks) ? j_lo + blocks_per_wg : n_blocks;
    for (uint64_t jb = j_lo + (uint64_t)wave * JW; jb < j_hi; jb += 8 * JW) {
        const uint64_t j = jb + jsub;  // block inside this launch: its output slot; CTR index first_block + j
        if (j >= j_hi) continue;
        uint32_t s[128], t[128];
        rounds_0_to_9<QW>(first_block + j, s, t, rkl);
        sub_shift(s, t);
        const uint32_t* rk10 = rkl + 10 * 128 * QW;
#pragma unroll
        for (int i = 0; i < 128; i++) t[i] ^= rk10[i * QW];
        // plane 8*i + k = bit k of keystream byte i; u64 h, bit b  <->  plane 64*h + b
#pragma unroll
        for (int h = 0; h < 2; h++) {
            uint32_t lo[32], hi[32];
#pragma unroll
            for (int k = 0; k < 32; k++) {
                lo[k] = t[64 * h + 31 - k];
                hi[k] = t[64 * h + 32 + 31 - k];
            }
            transpose32(lo);
            transpose32(hi);
            uint64_t* out = masks64 + (2 * j + h) * S + (uint64_t)q * 32;
#pragma unroll
            for (int sl = 0; sl < 32; sl++) {
                const uint32_t on = (uint32_t)0 - ((kp >> (31 - sl)) & 1u);  // omitted player's stream stays zero
                out[sl] = ((uint64_t)(hi[sl] & on) << 32) | (lo[sl] & on);
            }
        }
    }
