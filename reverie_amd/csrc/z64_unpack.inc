// The body of k_unpack64, textually shared with its recordable form B_k_unpack64 (z64.hip; see z64_interp.inc for why)
    const uint64_t tid = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const uint64_t it = tid / out_r;
    const uint32_t r = (uint32_t)(tid % out_r);
    if (it >= n_items) return;
    uint64_t v = 0;
    if (omit[r] < 8 && (it + 1) * 8 <= src_len[r]) {
        const uint8_t* s = blob + src_off[r] + 8 * it;
#pragma unroll
        for (int i = 0; i < 8; i++) v |= (uint64_t)s[i] << (8 * i);
    }
    out[it * out_r + r] = v;
