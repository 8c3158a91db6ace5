// compile_dev.hip, part 3: the split of a mixed list and its Z64 ops
static_assert(sizeof(Gate64) == 64, "Gate64 is compared bytewise: no padding");
struct Seeds64 {
    uint32_t ssa_base;  // the first op's SSA id: 1, or 1 + z64_wires behind a chunk's carried slots
    uint32_t m0;        // ShareGen<Z64> calls before the piece (mask64_phase)
    uint64_t on0, pre0;  // transcript words in front of the piece's own
};

// pc: {GF(2) op, Z64 op, 0, 0} -- their exclusive scan is every op's place in its domain's list; zc: the Z64 counters of compile.cpp
// (m: Input 1, Random 1, Mul 2; mul; as; in).  A B2A op, an unknown domain, a SizeHint that grows a wire count and any Z64 op
// run_pass rejects raise the flag: the host compiler takes the list.
// admit_b2a: a B2A op is {442 entries of the GF(2) list, one of the Z64 list, one B2A} in pc and one Z64 mask in zc, checked as
// run_pass checks it (dst in the Z64 wires, the 64 source wires in the GF(2) wires).
__global__ __launch_bounds__(TB) void k_z_classify(const rv_op* ops, size_t n, uint32_t W2, uint32_t W64, uint32_t admit_b2a, C4* zc, C4* pc, uint32_t* flag) {
    const size_t i = (size_t)blockIdx.x * TB + threadIdx.x;
    if (i >= n) return;
    const rv_op op = ops[i];
    bool bad = op.reserved != 0;
    C4 z{0, 0, 0, 0}, p{0, 0, 0, 0};
    if (op.domain == RV_DOM_GF2) {
        p.m = 1;
    } else if (op.domain == RV_DOM_Z64) {
        if (op.opcode > RV_OP_CONST) bad = true;
        const int nr = bad ? 0 : op_reads(op.opcode);
        if (!bad && op_writes(op.opcode) && op.dst >= W64) bad = true;
        if (nr >= 1 && op.a >= W64) bad = true;
        if (nr >= 2 && op.b >= W64) bad = true;
        p.mul = 1;
        if (op.opcode == RV_OP_INPUT) z.m = 1, z.in = 1;
        else if (op.opcode == RV_OP_RANDOM) z.m = 1;
        else if (op.opcode == RV_OP_MUL) z.m = 2, z.mul = 1;
        else if (op.opcode == RV_OP_ASSERTZERO) z.as = 1;
    } else if (op.domain == RV_DOM_SIZEHINT) {
        if (op.a > W64 || op.b > W2) bad = true;
    } else if (op.domain == RV_DOM_B2A && admit_b2a) {
        if (op.dst >= W64 || (uint64_t)op.a + 64 > W2) bad = true;
        p.m = B2A_STEPS, p.mul = 1, p.as = 1;
        z.m = 1;
    } else {
        bad = true;
    }
    if (bad) atomicOr(flag, 1u);
    zc[i] = z;
    pc[i] = p;
}
// px, zx: the exclusive scans.  Each domain's ops in order, with their places in the whole list; the Z64 ops' counters go with them
// A B2A goes into the Z64 list as a ZOP_B2A record whose `a` is the place of its expansion in the GF(2) list (k_z_expand fills that);
// bx64 (null: a list without B2A): the B2A ops in front of every Z64-list entry -- they share the correction ordinal with Mul;
// b2a: per B2A {its expansion's place, its first source wire, its place in the whole list}
__global__ __launch_bounds__(TB) void k_z_compact(const rv_op* ops, size_t n, const C4* px, const C4* zx, rv_op* ops2, uint32_t* orig2, rv_op* ops64,
                                                  uint32_t* orig64, C4* zc64, uint32_t* bx64, uint32_t* b2a_base, uint2* b2a_src) {
    const size_t i = (size_t)blockIdx.x * TB + threadIdx.x;
    if (i >= n) return;
    const rv_op op = ops[i];
    const C4 p = px[i];
    if (op.domain == RV_DOM_GF2) {
        ops2[p.m] = op;
        orig2[p.m] = (uint32_t)i;
    } else if (op.domain == RV_DOM_Z64 || op.domain == RV_DOM_B2A) {
        rv_op o = op;
        if (op.domain == RV_DOM_B2A) {
            o.domain = RV_DOM_Z64, o.opcode = ZOP_B2A, o.reserved = 0, o.a = p.m, o.b = 0, o.imm = 0;
            b2a_base[p.as] = p.m;
            b2a_src[p.as] = make_uint2(op.a, (uint32_t)i);
        }
        ops64[p.mul] = o;
        orig64[p.mul] = (uint32_t)i;
        zc64[p.mul] = zx[i];
        if (bx64) bx64[p.mul] = p.as;
    }
}
// Step j of a B2A's expansion (run_pass, case RV_DOM_B2A, in Builder::g_* call order) at place B of the GF(2) list, S = its first source
// wire: 64 Random a_k; Mul(a_0, b_0), Xor(a_0, b_0); for k = 1..62 ac = Xor(a_k, carry), bc = Xor(b_k, carry), t = Mul(ac, bc),
// res_k = Xor(ac, b_k), carry = Xor(t, carry); Xor(a_63, b_63), res_63 = Xor(carry, that); 64 reconstructions of res_k
__device__ inline rv_op b2a_step(uint32_t B, uint32_t S, uint32_t j) {
    rv_op o;
    o.domain = RV_DOM_GF2, o.opcode = RV_OP_ADD, o.reserved = PS_OP | PS_A | PS_B, o.dst = 0, o.a = 0, o.b = 0, o.imm = 0;
    if (j < 64) {
        o.opcode = RV_OP_RANDOM, o.reserved = PS_OP;
    } else if (j == 64 || j == 65) {
        o.opcode = j == 64 ? RV_OP_MUL : RV_OP_ADD;
        o.reserved = PS_OP | PS_A, o.a = B, o.b = S;
    } else if (j < 376) {
        const uint32_t k = 1 + (j - 66) / 5, t = (j - 66) % 5, at = 66 + 5 * (k - 1), carry = k == 1 ? 64u : at - 1;
        if (t == 0) o.a = B + k, o.b = B + carry;
        else if (t == 1) o.reserved = PS_OP | PS_B, o.a = S + k, o.b = B + carry;
        else if (t == 2) o.opcode = RV_OP_MUL, o.a = B + at, o.b = B + at + 1;
        else if (t == 3) o.reserved = PS_OP | PS_A, o.a = B + at, o.b = S + k;
        else o.a = B + at + 2, o.b = B + carry;
    } else if (j == 376) {
        o.reserved = PS_OP | PS_A, o.a = B + 63, o.b = S + 63;
    } else if (j == 377) {
        o.a = B + 375, o.b = B + 376;
    } else {
        const uint32_t k = j - B2A_RECON0;
        o.opcode = RV_OP_ASSERTZERO, o.reserved = PS_OP | PS_A;
        o.a = B + (k == 0 ? 65u : k == 63 ? 377u : 66 + 5 * (k - 1) + 3);
    }
    return o;
}
static_assert(66 + 5 * 62 == 376 && B2A_RECON0 + 64 == B2A_STEPS, "the steps of one B2A");
// one workgroup per B2A
__global__ __launch_bounds__(TB) void k_z_expand(const uint32_t* b2a_base, const uint2* b2a_src, rv_op* ops2, uint32_t* orig2) {
    const uint32_t B = b2a_base[blockIdx.x];
    const uint2 s = b2a_src[blockIdx.x];
    for (uint32_t j = threadIdx.x; j < B2A_STEPS; j += TB) {
        ops2[B + j] = b2a_step(B, s.x, j);
        orig2[B + j] = s.y;
    }
}
// a B2A gate's level, before the Z64 rounds: one above its deepest reconstruction (glvl2: the GF(2) list's gate levels)
__global__ __launch_bounds__(TB) void k_z_b2a_levels(const rv_op* ops64, size_t n, const int* glvl2, int* glvl) {
    const size_t i = (size_t)blockIdx.x * TB + threadIdx.x;
    if (i >= n) return;
    const rv_op op = ops64[i];
    if (op.opcode != ZOP_B2A) return;
    int l = 0;
    for (uint32_t k = 0; k < 64; k++) l = max(l, glvl2[op.a + B2A_RECON0 + k]);
    glvl[i] = l + 1;
}
// the writer sort's keys (as k_cd_classify's: the wire, W64 for AssertZero)
__global__ __launch_bounds__(TB) void k_z_wkeys(const rv_op* ops, size_t n, uint32_t W64, uint32_t* keys, uint32_t* vals) {
    const size_t i = (size_t)blockIdx.x * TB + threadIdx.x;
    if (i >= n) return;
    const rv_op op = ops[i];
    keys[i] = op_writes(op.opcode) ? op.dst : W64;
    vals[i] = (uint32_t)i;
}
// the level sort's keys, and the deepest level (one atomic per wavefront)
__global__ __launch_bounds__(TB) void k_z_lkeys(const int* glvl, size_t n, uint32_t* keys, uint32_t* vals, uint32_t* max_level) {
    const size_t i = (size_t)blockIdx.x * TB + threadIdx.x;
    const uint32_t l = i < n ? (uint32_t)glvl[i] : 0u;
    if (i < n) {
        keys[i] = l;
        vals[i] = (uint32_t)i;
    }
    const uint32_t m = wave_max_u32(l);
    if ((threadIdx.x & 63u) == 0 && m) atomicMax(max_level, m);
}
// a chunk's written wires (each gets a write-back: an op's SSA id is never the carried slot's)
__global__ __launch_bounds__(TB) void k_z_wb_flags(const uint32_t* seg_lo, const uint32_t* seg_hi, uint32_t W64, uint32_t* fl) {
    const size_t w = (size_t)blockIdx.x * TB + threadIdx.x;
    if (w >= W64) return;
    fl[w] = seg_hi[w] > seg_lo[w];
}
// an operand: its SSA id (never written: 0; a chunk's carried slot 1 + w) and where its mask row lives (Builder::emit64's ssa_row64)
__device__ inline uint32_t z_ssa(int p, const C4* zc, const Seeds64& s) {
    return p >= 0 ? s.ssa_base + (uint32_t)p - zc[p].as : p == -1 ? 0u : 1u + (uint32_t)(-2 - p);
}
__device__ inline uint32_t z_mask_row(int p, const rv_op* ops, const C4* zc, const Seeds64& s) {
    if (p >= 0) {
        const uint32_t opc = ops[p].opcode;
        if (opc == RV_OP_INPUT || opc == RV_OP_RANDOM) return G64_MASK_ROW | (s.m0 + zc[p].m);
        if (opc == RV_OP_MUL) return G64_MASK_ROW | (s.m0 + zc[p].m + 1);
    }
    return z_ssa(p, zc, s);
}
// the Gate64 records in (level, program) order; the input / reconstruction offsets and the AssertZero tables by ordinal
// (bx: the B2A ops in front of each op, null without any; b2a_rows: Mixed::b2a_rows)
__global__ __launch_bounds__(TB) void k_z_gates(const uint32_t* sv, size_t n, const rv_op* ops, const int2* prod, const C4* zc, const uint32_t* orig, Seeds64 s,
                                                const uint32_t* bx, const uint32_t* b2a_rows, Gate64* gates, uint64_t* rec_offs, uint64_t* in_offs,
                                                uint32_t* as_rec, uint64_t* as_op) {
    const size_t p = (size_t)blockIdx.x * TB + threadIdx.x;
    if (p >= n) return;
    const uint32_t i = sv[p];
    const rv_op op = ops[i];
    const C4 c = zc[i];
    const int2 pr = prod[i];
    const int nr = op_reads(op.opcode);
    Gate64 g;
    g.op = 0, g.dst = 0, g.a = 0, g.b = 0, g.m = 0, g.m2 = 0, g.eo = 0, g.ep = 0, g.x = 0, g.xc = 0;
    g.imm = op.imm;
    g.a = nr >= 1 ? z_ssa(pr.x, zc, s) : 0u;
    g.b = nr >= 2 ? z_ssa(pr.y, zc, s) : 0u;
    g.am = nr >= 1 ? z_mask_row(pr.x, ops, zc, s) : 0u;
    g.bm = nr >= 2 ? z_mask_row(pr.y, ops, zc, s) : 0u;
    if (op_writes(op.opcode)) g.dst = s.ssa_base + i - c.as;
    const uint64_t eo = s.on0 + c.in + 8ull * ((uint64_t)c.mul + c.as);
    const uint32_t x = c.mul + c.as;
    const uint32_t nb = bx ? bx[i] : 0u, corr = c.mul + nb;  // corrections so far: Mul and B2A
    switch (op.opcode) {
    case ZOP_B2A:
        g.op = G64_B2A;
        g.a = b2a_rows[2 * nb];
        g.m = s.m0 + c.m;
        g.m2 = b2a_rows[2 * nb + 1];
        g.ep = s.pre0 + corr;
        g.xc = corr;
        break;
    case RV_OP_INPUT:
        g.op = G64_INPUT;
        g.m = s.m0 + c.m;
        g.eo = eo;
        g.x = c.in;
        in_offs[c.in] = eo;
        break;
    case RV_OP_RANDOM:
        g.op = G64_RANDOM;
        g.m = s.m0 + c.m;
        break;
    case RV_OP_CONST: g.op = G64_CONST; break;
    case RV_OP_ADD: g.op = G64_ADD; break;
    case RV_OP_SUB: g.op = G64_SUB; break;
    case RV_OP_ADDCONST: g.op = G64_ADDC; break;
    case RV_OP_SUBCONST: g.op = G64_SUBC; break;
    case RV_OP_MULCONST: g.op = G64_MULC; break;
    case RV_OP_MUL:
        g.op = G64_MUL;
        g.m = s.m0 + c.m;
        g.ep = s.pre0 + corr;
        g.xc = corr;
        g.eo = eo;
        g.x = x;
        rec_offs[x] = eo;
        break;
    default:  // AssertZero
        g.op = G64_ASSERT;
        g.eo = eo;
        g.x = x;
        rec_offs[x] = eo;
        as_rec[c.as] = x;
        as_op[c.as] = orig ? orig[i] : i;
        break;
    }
    gates[p] = g;
}
// a chunk's write-back level: wire w's final value copied to its carried slot.  sv: the writer sort's op indices; fx: the exclusive
// scan of k_z_wb_flags
__global__ __launch_bounds__(TB) void k_z_wb_gates(const uint32_t* sv, const uint32_t* seg_lo, const uint32_t* seg_hi, const uint32_t* fx, uint32_t W64,
                                                   const rv_op* ops, const C4* zc, Seeds64 s, Gate64* gates) {
    const size_t w = (size_t)blockIdx.x * TB + threadIdx.x;
    if (w >= W64 || seg_hi[w] <= seg_lo[w]) return;
    const int q = (int)sv[seg_hi[w] - 1];
    Gate64 g;
    g.op = G64_ADDC, g.dst = 1u + (uint32_t)w, g.b = 0, g.m = 0, g.m2 = 0, g.eo = 0, g.ep = 0, g.x = 0, g.xc = 0, g.imm = 0, g.bm = 0;
    g.a = z_ssa(q, zc, s);
    g.am = z_mask_row(q, ops, zc, s);
    gates[fx[w]] = g;
}
// RV_COMPILE_KEEP_WIRES: wire w's final SSA id, Builder::cur64 at the end of the program (a never-written wire: 0; a wire a B2A
// wrote last: that Gate64's dst, numbered like any other op's)
__global__ __launch_bounds__(TB) void k_z_wire_ssa(const uint32_t* sv, const uint32_t* seg_lo, const uint32_t* seg_hi, uint32_t W64, const C4* zc, Seeds64 s,
                                                   uint32_t* ssa) {
    const size_t w = (size_t)blockIdx.x * TB + threadIdx.x;
    if (w >= W64) return;
    ssa[w] = seg_hi[w] > seg_lo[w] ? z_ssa((int)sv[seg_hi[w] - 1], zc, s) : 0u;
}

// ---- the host phases ----
// the words the host reads back (zeroed once; the kernels get pointers to the members)
struct SplitWords {
    uint32_t flag;       // k_z_classify: an op the device path does not take, or an op-list error
    C4 tot;              // the Z64 counters' totals
    C4 count;            // m = entries of the GF(2) list, mul = of the Z64 list, as = B2A ops
    uint32_t max_level, n_wb;  // the deepest Z64 level; a chunk's Z64 write-backs
};
// One mixed compile's Z64 side between its phases (device arrays of the split's work Scratch)
struct Z64State {
    size_t n, n2, n64;  // ops of the whole list, entries of its GF(2) list (expansions included) and of its Z64 list
    const ChunkStart* chunk; uint32_t W64, n_b2a;
    C4 tot, *zc;
    Seeds64 s64; uint64_t n_masks64;
    SplitWords* d_words; rv_op *ops2, *ops64;
    uint32_t *orig2, *orig64, *bx64, *b2a_base, *b2a_rows;  // (the last three null: a list without B2A)
    // z64_levels
    Dag dag; int* glvl;
    uint32_t *wbx, *lk[2], *lv[2];  // a chunk: the exclusive scan of the written-wire flags; the level sort's buffers, keys and values filled
    uint32_t levels64, n_wb64;
    bool no_z64() const { return n2 == n && n64 == 0; }  // no Z64 op, no B2A and no SizeHint: the list as it is
};

// step 1: classify, split -- one thread per op of the whole list: the Z64 and SizeHint checks of run_pass (the GF(2) ops are checked by
// k_cd_classify once compacted), the Z64 counters and each op's place in its domain's list: two 16-byte tuple scans.  After RV_OK,
// z.no_z64() says the list is a GF(2) list as it stands.
int z64_split(Scratch& S, LapTimer& T, hipStream_t st, const DevCompileRequest& q, Z64State& z) {
    const size_t n = z.n = q.n_ops;
    const rv_op* d_ops = q.d_ops;
    const uint32_t gb = blocks(n, TB), W2 = (uint32_t)q.gf2_wires, W64 = z.W64 = (uint32_t)q.z64_wires;
    const ChunkStart* chunk = z.chunk = q.chunk;
    T.mark(LAP_SPLIT);
    C4* zx = S.get<C4>(n);
    C4* px = S.get<C4>(n);
    z.d_words = S.get<SplitWords>(1);
    CDNEED(zx && px && z.d_words);
    CDCHK(hipMemsetAsync(z.d_words, 0, sizeof(SplitWords), st));
    k_z_classify<<<gb, TB, 0, st>>>(d_ops, n, W2, W64, (q.device_bits & RV_COMPILE_DEVICE_B2A) ? 1u : 0u, zx, px, &z.d_words->flag);
    CDCHK(hipGetLastError());
    CDCHK((scan_excl<C4, SumC4>(S, st, zx, zx, n, &z.d_words->tot)));
    CDCHK((scan_excl<C4, SumC4>(S, st, px, px, n, &z.d_words->count)));
    SplitWords hw;
    CDCHK(hipMemcpyAsync(&hw, z.d_words, sizeof hw, hipMemcpyDeviceToHost, st));
    CDCHK(hipStreamSynchronize(st));
    if (hw.flag) return RV_COMPILE_FALLBACK;
    const C4 tot = z.tot = hw.tot;
    const uint32_t n_b2a = z.n_b2a = hw.count.as;
    if ((uint64_t)n_b2a * B2A_STEPS >= (1u << 28)) return RV_COMPILE_FALLBACK;  // (the expanded GF(2) list: below 2^28 entries, and no sum above wrapped)
    const size_t n2 = z.n2 = hw.count.m, n64 = z.n64 = hw.count.mul;
    if (z.no_z64()) return RV_OK;
    z.s64 = Seeds64{1u + (chunk ? W64 : 0u), chunk ? chunk->mask64_phase : 0u, chunk ? chunk->on_words64_0 : 0, chunk ? chunk->pre_words64_0 : 0};
    z.n_masks64 = (uint64_t)z.s64.m0 + tot.m;
    if ((uint64_t)z.s64.ssa_base + n64 > LIM || z.n_masks64 > LIM || (z.n_masks64 + 1) / 2 > RV_MAX_CTR_BLOCKS) return RV_COMPILE_FALLBACK;
    z.ops2 = S.get<rv_op>(n2);
    z.orig2 = S.get<uint32_t>(n2);
    z.ops64 = S.get<rv_op>(n64);
    z.orig64 = S.get<uint32_t>(n64);
    z.zc = S.get<C4>(n64);
    CDNEED(z.ops2 && z.orig2 && z.ops64 && z.orig64 && z.zc);
    uint2* b2a_src = nullptr;
    if (n_b2a) {
        z.bx64 = S.get<uint32_t>(n64);
        z.b2a_base = S.get<uint32_t>(n_b2a);
        b2a_src = S.get<uint2>(n_b2a);
        z.b2a_rows = S.get<uint32_t>(2 * (size_t)n_b2a);
        CDNEED(z.bx64 && z.b2a_base && b2a_src && z.b2a_rows);
    }
    k_z_compact<<<gb, TB, 0, st>>>(d_ops, n, px, zx, z.ops2, z.orig2, z.ops64, z.orig64, z.zc, z.bx64, z.b2a_base, b2a_src);
    if (n_b2a) k_z_expand<<<n_b2a, TB, 0, st>>>(z.b2a_base, b2a_src, z.ops2, z.orig2);
    CDCHK(hipGetLastError());
    T.mark(LAP_SPLIT_END);
    return RV_OK;
}

// steps 2 and 3: the Z64 ops' writers (build_dag) and levels (the round kernel in its FORM_Z64), run once the GF(2) ops have theirs
// (glvl2: the level of every GF(2) op's gate) -- a B2A gate sits one level above its deepest reconstruction.  Then a chunk's written
// wires and the level sort's keys.
int z64_levels(Scratch& S, LapTimer& T, hipStream_t st, Z64State& z, const int* glvl2) {
    const size_t n64 = z.n64;
    if (!n64) return RV_OK;
    const uint32_t W64 = z.W64, gb64 = blocks(n64, TB);
    T.mark(LAP_Z64_LEVELS);
    uint32_t *kbuf[2], *vbuf[2];
    for (int k = 0; k < 2; k++) kbuf[k] = S.get<uint32_t>(n64);
    for (int k = 0; k < 2; k++) vbuf[k] = S.get<uint32_t>(n64);
    CDNEED(kbuf[0] && kbuf[1] && vbuf[0] && vbuf[1]);
    k_z_wkeys<<<gb64, TB, 0, st>>>(z.ops64, n64, W64, kbuf[0], vbuf[0]);
    CDCHK(hipGetLastError());
    if (const int rc = build_dag(S, st, z.ops64, n64, W64, z.chunk ? 1u : 0u, kbuf, vbuf, z.dag)) return rc;
    const Dag& d = z.dag;
    z.glvl = S.get<int>(n64);
    CDNEED(z.glvl);
    if (z.n_b2a) k_z_b2a_levels<<<gb64, TB, 0, st>>>(z.ops64, n64, glvl2, z.glvl);
    CDCHK(hipGetLastError());
    uint32_t r = 0;
    if (const int rc = run_rounds(st, FORM_Z64, 0u, z.ops64, n64, d, nullptr, nullptr, z.glvl, nullptr, &r)) return rc;
    if (z.chunk) {
        z.wbx = S.get<uint32_t>(W64);
        CDNEED(z.wbx);
        k_z_wb_flags<<<blocks(W64, TB), TB, 0, st>>>(d.seg_lo, d.seg_hi, W64, z.wbx);
        CDCHK(hipGetLastError());
        CDCHK((scan_excl<uint32_t, SumU32>(S, st, z.wbx, z.wbx, W64, &z.d_words->n_wb)));
    }
    // the level sort's keys (the writer sort's values stay in d.sv for the write-back gates; its other three buffers are free)
    z.lk[0] = kbuf[d.which], z.lk[1] = kbuf[d.which ^ 1];
    z.lv[0] = vbuf[d.which ^ 1], z.lv[1] = S.get<uint32_t>(n64);
    CDNEED(z.lv[1]);
    k_z_lkeys<<<gb64, TB, 0, st>>>(z.glvl, n64, z.lk[0], z.lv[0], &z.d_words->max_level);
    CDCHK(hipGetLastError());
    SplitWords hw;
    CDCHK(hipMemcpyAsync(&hw, z.d_words, sizeof hw, hipMemcpyDeviceToHost, st));
    CDCHK(hipStreamSynchronize(st));
    z.levels64 = hw.max_level + 1;
    z.n_wb64 = z.chunk ? hw.n_wb : 0;
    T.mark(LAP_Z64_LEVELS_END);
    return RV_OK;
}

// the Z64 fields of the host's tables (cc: what gf2_tables made of the GF(2) list)
void z64_fill(Compiled& cc, const Z64State& z, uint64_t n_g64) {
    const C4 tot = z.tot;
    const uint64_t n_rec64 = (uint64_t)tot.mul + tot.as, n_b2a = z.n_b2a;
    cc.level_start64.back() = (uint32_t)n_g64;  // (the write-backs: the last level's, behind every op's gate)
    const uint64_t randoms = (uint64_t)tot.m - tot.in - 2ull * tot.mul - n_b2a;  // (a B2A's Z64 mask is not a Random op)
    cc.n_ssa64 = (uint64_t)z.s64.ssa_base + z.n64 - tot.as, cc.n_masks64 = z.n_masks64;
    cc.on_words64 = z.s64.on0 + tot.in + 8 * n_rec64, cc.pre_words64 = z.s64.pre0 + tot.mul + n_b2a;
    cc.n_in64 = tot.in, cc.n_rec64 = n_rec64, cc.n_corr64 = (uint64_t)tot.mul + n_b2a;
    cc.n_user_random += randoms;
    cc.info.z64_inputs = tot.in, cc.info.z64_muls = tot.mul, cc.info.z64_asserts = tot.as;
    cc.info.z64_linear = (uint64_t)z.n64 - tot.in - tot.mul - tot.as - n_b2a + z.n_wb64;
    cc.info.z64_masks = z.n_masks64, cc.info.b2a = z.n_b2a;
}

// RV_COMPILE_KEEP_WIRES: Compiled::wire_ssa64 and its device copy (the result Scratch's), from the writers sort of the Z64 list
// (z null or without Z64 entries: every wire reads as SSA 0).  Synchronises the stream.
int z64_wire_table(Scratch& S, Scratch& R, hipStream_t st, const Z64State* z, size_t z64_wires, Compiled& cc, uint32_t** d_out) {
    const uint32_t W64 = (uint32_t)z64_wires;
    if (!W64) return RV_OK;
    uint32_t* ssa = *d_out = R.get<uint32_t>(W64);
    CDNEED(ssa);
    if (z && z->n64) k_z_wire_ssa<<<blocks(W64, TB), TB, 0, st>>>(z->dag.sv, z->dag.seg_lo, z->dag.seg_hi, W64, z->zc, z->s64, ssa);
    else CDCHK(hipMemsetAsync(ssa, 0, (size_t)W64 * 4, st));
    CDCHK(hipGetLastError());
    cc.wire_ssa64.resize(W64);
    CDCHK(fetch(st, cc.wire_ssa64, ssa));
    CDCHK(hipStreamSynchronize(st));
    return RV_OK;
}

// step 4: the Z64 tables, into the Compiled gf2_tables filled (its level count is both domains') -- a stable sort by level; the records,
// offsets and AssertZero tables written by one thread per gate; a chunk's write-back copies (one G64_ADDC per written wire, in wire
// order) behind them.  res: gates64 and the two offset tables, the result Scratch's.
int z64_tables(Scratch& S, Scratch& R, LapTimer& T, hipStream_t st, Z64State& z, bool keep_wires, Compiled& cc, DevCompileKeep& res) {
    const uint32_t n_levels = (uint32_t)cc.level_start.size() - 1, W64 = z.W64;
    cc.level_start64.assign((size_t)n_levels + 1, 0);
    const size_t n64 = z.n64;
    if (!n64) return keep_wires ? z64_wire_table(S, R, st, &z, W64, cc, &res.d_wire_ssa64) : RV_OK;
    if (n_levels < z.levels64 + (z.n_wb64 ? 1u : 0u)) return RV_E_DEVICE;  // (cannot happen)
    T.mark(LAP_Z64_TABLES);
    const C4 tot = z.tot;
    const Dag& d = z.dag;
    const uint64_t n_rec64 = (uint64_t)tot.mul + tot.as, n_g64 = (uint64_t)n64 + z.n_wb64;
    Gate64* gates64 = res.d_gates64 = R.get<Gate64>(n_g64);
    uint64_t* rec_offs = res.d_rec_offs64 = R.get<uint64_t>(n_rec64);
    uint64_t* in_offs = res.d_in_offs64 = R.get<uint64_t>(tot.in);
    uint32_t* as_rec = S.get<uint32_t>(tot.as);
    uint64_t* as_op = S.get<uint64_t>(tot.as);
    uint32_t* pos = S.get<uint32_t>((size_t)n_levels + 1);
    CDNEED(gates64 && rec_offs && in_offs && as_rec && as_op && pos);
    if (z.n_wb64) k_z_wb_gates<<<blocks(W64, TB), TB, 0, st>>>(d.sv, d.seg_lo, d.seg_hi, z.wbx, W64, z.ops64, z.zc, z.s64, gates64 + n64);
    int lsort = 0;
    CDCHK(radix_sort(S, st, z.lk, z.lv, n64, bit_len(z.levels64), &lsort));
    k_cd_bounds<<<blocks(n64 + 1, TB), TB, 0, st>>>(z.lk[lsort], n64, n_levels, pos);
    k_z_gates<<<blocks(n64, TB), TB, 0, st>>>(z.lv[lsort], n64, z.ops64, d.prod, z.zc, z.orig64, z.s64, z.bx64, z.b2a_rows, gates64, rec_offs, in_offs, as_rec, as_op);
    CDCHK(hipGetLastError());
    cc.gates64.resize(n_g64);
    cc.rec_offs64.resize(n_rec64);
    cc.in_offs64.resize(tot.in);
    cc.assert_rec64.resize(tot.as);
    cc.assert_op64.resize(tot.as);
    CDCHK(fetch(st, cc.gates64, gates64));
    CDCHK(fetch(st, cc.rec_offs64, rec_offs));
    CDCHK(fetch(st, cc.in_offs64, in_offs));
    CDCHK(fetch(st, cc.assert_rec64, as_rec));
    CDCHK(fetch(st, cc.assert_op64, as_op));
    CDCHK(fetch(st, cc.level_start64, pos));
    if (keep_wires)
        if (const int rc = z64_wire_table(S, R, st, &z, W64, cc, &res.d_wire_ssa64)) return rc;
    T.mark(LAP_Z64_TABLES_END);
    CDCHK(hipStreamSynchronize(st));
    z64_fill(cc, z, n_g64);
    return RV_OK;
}
