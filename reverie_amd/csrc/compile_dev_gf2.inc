// compile_dev.hip, part 2: the GF(2) pipeline (its DAG and round kernels serve the Z64 ops as well)
constexpr uint32_t MAX_ROUNDS = 1u << 16;  // topological rounds before the host compiler takes over

// the counters of one op (compile.cpp Builder): ShareGen::next() calls, Mul gates, AssertZero gates, Input gates
struct C4 {
    uint32_t m, mul, as, in;
};
struct SumC4 {
    __device__ C4 operator()(const C4& a, const C4& b) const { return C4{a.m + b.m, a.mul + b.mul, a.as + b.as, a.in + b.in}; }
    static __device__ C4 id() { return C4{0, 0, 0, 0}; }
};
// what a streaming chunk adds to the kernels' numbering (all zero: a whole program)
struct Seeds {
    uint32_t chunk;    // 1: chunk mode
    uint32_t base;     // carried rows in front of the PRG rows (row_prg_base)
    uint32_t m0;       // ShareGen calls before the piece, modulo 128
    uint32_t on0, pre0;  // transcript rows in front of the piece's own
    uint32_t n_wbmat;  // carried forms materialised for the write-back level (level 0, class 3)
};

// ---- the op list ----
// The private ops of a B2A expansion (RV_COMPILE_DEVICE_B2A; k_z_expand writes them into the GF(2) list of a mixed compile, nobody
// else may): GF(2) records whose `reserved` word says PS_OP = writes no wire (sort key W), PS_A / PS_B = operand a / b names its
// producer by its place in the list instead of a wire.  A PS_OP AssertZero is Builder::g_reveal(recon = true): the gate is a G_RECON
// and has a value, a fresh computed row.
constexpr uint16_t PS_OP = 1, PS_A = 2, PS_B = 4;
constexpr uint32_t B2A_STEPS = 442, B2A_RECON0 = 378;  // SSA-producing steps of one B2A (run_pass); its first reconstruction
constexpr uint8_t ZOP_B2A = RV_OP_CONST + 1;           // the B2A's record in the Z64 list (a = its expansion's place in the GF(2) list)
__device__ inline bool is_recon(const rv_op& op) { return op.opcode == RV_OP_ASSERTZERO && (op.reserved & PS_OP); }
__device__ inline bool op_writes(uint32_t opc) { return opc != RV_OP_ASSERTZERO; }
__device__ inline int op_reads(uint32_t opc) {
    switch (opc) {
    case RV_OP_ADD: case RV_OP_SUB: case RV_OP_MUL: return 2;
    case RV_OP_ADDCONST: case RV_OP_SUBCONST: case RV_OP_MULCONST: case RV_OP_ASSERTZERO: return 1;
    default: return 0;
    }
}

// step 1: validation, counters, the wire sort's keys (a wire; W for ops that write none: they sort behind every wire)
// (pseudo: the list is a mixed compile's own and may hold the private ops of B2A expansions)
__global__ __launch_bounds__(TB) void k_cd_classify(const rv_op* ops, size_t n, uint32_t W, uint32_t pseudo, C4* cnt, uint32_t* keys, uint32_t* vals,
                                                    uint32_t* flag) {
    const size_t i = (size_t)blockIdx.x * TB + threadIdx.x;
    if (i >= n) return;
    const rv_op op = ops[i];
    bool bad = op.domain != RV_DOM_GF2 || (pseudo ? (op.reserved & ~(PS_OP | PS_A | PS_B)) != 0 : op.reserved != 0) || op.opcode > RV_OP_CONST;
    const int nr = bad ? 0 : op_reads(op.opcode);
    const bool wr = !bad && op_writes(op.opcode) && !(op.reserved & PS_OP);
    if (wr && op.dst >= W) bad = true;
    if (nr >= 1 && !(op.reserved & PS_A) && op.a >= W) bad = true;
    if (nr >= 2 && !(op.reserved & PS_B) && op.b >= W) bad = true;
    if (bad) atomicOr(flag, 1u);
    C4 c{0, 0, 0, 0};
    if (!bad) {
        if (op.opcode == RV_OP_INPUT) c.m = 1, c.in = 1;
        else if (op.opcode == RV_OP_RANDOM) c.m = 1;
        else if (op.opcode == RV_OP_MUL) c.m = 2, c.mul = 1;
        else if (op.opcode == RV_OP_ASSERTZERO) c.as = 1;
    }
    cnt[i] = c;
    keys[i] = wr ? op.dst : W;
    vals[i] = (uint32_t)i;
}

// the ordinal tables: reconstruction ordinal -> online row, input ordinal -> online row, the AssertZero ops
// (b2a_base: where the n_b2a expansions start in the list, ascending.  Their reconstructions count in c.as like AssertZero ops but are
// not in the AssertZero tables: 64 per expansion in front of op i come off its ordinal there)
__global__ __launch_bounds__(TB) void k_cd_ordinals(const rv_op* ops, size_t n, const C4* cx, uint32_t on0, uint32_t* rec_rows, uint32_t* in_rows,
                                                    uint32_t* as_rec, uint64_t* as_op, const uint32_t* orig, const uint32_t* b2a_base, uint32_t n_b2a) {
    const size_t i = (size_t)blockIdx.x * TB + threadIdx.x;
    if (i >= n) return;
    const rv_op op = ops[i];
    const uint32_t opc = op.opcode;
    const C4 c = cx[i];
    const uint32_t eo = on0 + c.in + c.mul + c.as, x = c.mul + c.as;
    if (opc == RV_OP_INPUT) in_rows[c.in] = eo;
    if (opc == RV_OP_MUL || opc == RV_OP_ASSERTZERO) rec_rows[x] = eo;
    if (opc == RV_OP_ASSERTZERO && !is_recon(op)) {
        uint32_t a = 0, b = n_b2a;
        while (a < b) {  // (expansions that start before op i; at most 32 steps)
            const uint32_t mid = a + (b - a) / 2;
            if (b2a_base[mid] < i) a = mid + 1;
            else b = mid;
        }
        const uint32_t k = c.as - 64u * a;
        as_rec[k] = x;
        as_op[k] = orig ? orig[i] : i;  // (orig: the ops are the GF(2) ops of a mixed list, orig[i] = op i's place in it)
    }
}

// step 2: each wire's segment of the sorted writes
__global__ __launch_bounds__(TB) void k_cd_segs(const uint32_t* sk, size_t n, uint32_t W, uint32_t* seg_lo, uint32_t* seg_hi) {
    const size_t p = (size_t)blockIdx.x * TB + threadIdx.x;
    if (p >= n) return;
    const uint32_t k = sk[p];
    if (k >= W) return;
    if (p == 0 || sk[p - 1] != k) seg_lo[k] = (uint32_t)p;
    if (p + 1 == n || sk[p + 1] != k) seg_hi[k] = (uint32_t)p + 1;
}
__device__ inline int last_writer(const uint32_t* sv, const uint32_t* seg_lo, const uint32_t* seg_hi, uint32_t w, uint32_t i) {
    uint32_t lo = seg_lo[w], a = lo, b = seg_hi[w];
    while (a < b) {  // (at most 32 steps)
        const uint32_t mid = a + (b - a) / 2;
        if (sv[mid] < i) a = mid + 1;
        else b = mid;
    }
    return a > lo ? (int)sv[a - 1] : -1;
}
// the producer of every operand (-1: the never-written wire; chunk mode: -2 - w, wire w's carried row), read counts, pending operands
__global__ __launch_bounds__(TB) void k_cd_resolve(const rv_op* ops, size_t n, const uint32_t* sv, const uint32_t* seg_lo, const uint32_t* seg_hi,
                                                   uint32_t chunk, int2* prod, uint32_t* uses, uint32_t* rem) {
    const size_t i = (size_t)blockIdx.x * TB + threadIdx.x;
    if (i >= n) return;
    const rv_op op = ops[i];
    const int nr = op_reads(op.opcode);
    int2 p = make_int2(-1, -1);
    // (a private op of a B2A expansion names the steps of its own expansion by their places; its reads of the source wires are
    // searched like any other: no step of an expansion writes a wire, so every place in it sees the B2A's own last writers)
    if (nr >= 1) p.x = (op.reserved & PS_A) ? (int)op.a : last_writer(sv, seg_lo, seg_hi, op.a, (uint32_t)i);
    if (nr >= 2) p.y = (op.reserved & PS_B) ? (int)op.b : last_writer(sv, seg_lo, seg_hi, op.b, (uint32_t)i);
    if (chunk) {
        if (nr >= 1 && p.x < 0) p.x = -2 - (int)op.a;
        if (nr >= 2 && p.y < 0) p.y = -2 - (int)op.b;
    }
    uint32_t r = 0;
    if (p.x >= 0) atomicAdd(&uses[p.x], 1u), r++;
    if (p.y >= 0) atomicAdd(&uses[p.y], 1u), r++;
    prod[i] = p;
    rem[i] = r;
}
__global__ __launch_bounds__(TB) void k_cd_consumers(const int2* prod, size_t n, const uint32_t* cons_off, uint32_t* cursor, uint32_t* cons) {
    const size_t i = (size_t)blockIdx.x * TB + threadIdx.x;
    if (i >= n) return;
    const int2 p = prod[i];
    if (p.x >= 0) cons[cons_off[p.x] + atomicAdd(&cursor[p.x], 1u)] = (uint32_t)i;
    if (p.y >= 0) cons[cons_off[p.y] + atomicAdd(&cursor[p.y], 1u)] = (uint32_t)i;
}
// round 0's frontier: the ops with no pending operand
__global__ __launch_bounds__(TB) void k_cd_front0(const uint32_t* rem, size_t n, uint32_t* frontier, uint2* rounds) {
    const size_t i = (size_t)blockIdx.x * TB + threadIdx.x;
    if (i >= n) return;
    if (rem[i] == 0) frontier[atomicAdd(&rounds[0].y, 1u)] = (uint32_t)i;
}

// a value: x = the op that wrote its row (-1: a constant; -2 - w: wire w's carried row, there before level 0),
// y = (level of that row + 1) << 1 | constant bit
__device__ inline int2 val_of(const int2* V, int p) { return p < 0 ? make_int2(p, 0) : V[p]; }
__device__ inline int lvl_of(int2 v) { return (v.y >> 1) - 1; }
__device__ inline bool is_row(int2 v) { return v.x != -1; }

// ---- the lazy-sum form (force_lazy_k = RV_LIN_K; whole programs only) ----
// A value is a Lin of compile.cpp: x, y, z = up to RV_LIN_K rows in the host compiler's order, w = count | constant bit << 2 (the
// value of a materialised sum also keeps that gate's row count, << 8, for the statistics and the class keys).  A row is named by the
// op that wrote it, with ROW_COMP set when that op is a materialised sum: the host compiler sorts PRG rows (mask index) before
// computed rows (COMP | index), and both indices grow in op order, so comparing these names compares its row numbers.
// A row's level is glvl of its op; a never-written wire is the empty form.
static_assert(RV_LIN_K == 3, "a lazy value holds three rows");
constexpr uint32_t ROW_COMP = 1u << 30;  // (n_ops < 2^28)
__device__ inline uint4 form_of(const uint4* V3, int p) { return p < 0 ? make_uint4(0, 0, 0, 0) : V3[p]; }
__device__ inline uint32_t form_n(const uint4& F) { return F.w & 3u; }
__device__ inline uint32_t form_c(const uint4& F) { return (F.w >> 2) & 1u; }
__device__ inline uint32_t form_row(const uint4& F, int k) { return k == 0 ? F.x : k == 1 ? F.y : F.z; }
__device__ inline int form_lvl(const uint4& F, const int* glvl) {
    const uint32_t n = form_n(F);
    int l = -1;
    if (n > 0) l = max(l, glvl[F.x & ~ROW_COMP]);
    if (n > 1) l = max(l, glvl[F.y & ~ROW_COMP]);
    if (n > 2) l = max(l, glvl[F.z & ~ROW_COMP]);
    return l;
}
// Builder::g_xor's symmetric difference of two sorted row lists (x ^ x = 0): at most 6 rows, one or two consumed per step
__device__ inline int form_xor(const uint4& A, const uint4& B, uint32_t (&rows)[2 * RV_LIN_K]) {
    const int na = (int)form_n(A), nb = (int)form_n(B);
    int i = 0, j = 0, n = 0;
#pragma unroll
    for (int k = 0; k < 2 * RV_LIN_K; k++) rows[k] = 0;
#pragma unroll
    for (int t = 0; t < 2 * RV_LIN_K; t++) {
        if (i < na || j < nb) {
            const uint32_t x = i < na ? form_row(A, i) : 0xFFFFFFFFu, y = j < nb ? form_row(B, j) : 0xFFFFFFFFu;
            if (x == y) {
                i++, j++;
            } else {
                const uint32_t v = min(x, y);
                i += x < y, j += y < x;
#pragma unroll
                for (int k = 0; k < 2 * RV_LIN_K; k++)
                    if (n == k) rows[k] = v;
                n++;
            }
        }
    }
    return n;
}

// the value of op i, the level of its gate (-1: none) and whether it is a materialised sum: the rules of Builder::g_xor / g_xorc /
// g_andc / g_const / g_mul at lazy_k = 1 ...
__device__ inline int2 value_k1(const rv_op& op, uint32_t i, int2 p, uint32_t chunk, const uint32_t* uses, const int2* V, int* gl, uint32_t* mt) {
    const int2 A = val_of(V, p.x), B = val_of(V, p.y);
    const int cb = (int)(op.imm & 1);
    int2 out = make_int2(-1, 0);
    switch (op.opcode) {
    case RV_OP_INPUT:
    case RV_OP_RANDOM:
        *gl = 0;
        out = make_int2((int)i, 1 << 1);
        break;
    case RV_OP_CONST:
        out = make_int2(-1, cb);
        break;
    case RV_OP_ADD:
    case RV_OP_SUB:
        if (A.x == B.x) out = make_int2(-1, (A.y ^ B.y) & 1);       // x ^ x = 0 (or two constants)
        else if (!is_row(A)) out = make_int2(B.x, B.y ^ (A.y & 1));  // a constant plus a row: the row
        else if (!is_row(B)) out = make_int2(A.x, A.y ^ (B.y & 1));
        else if (!chunk && uses[i] == 0) out = make_int2(-1, 0);    // an unread sum is dropped (a chunk counts no reads)
        else {                                                      // two rows: a G_XORK
            *gl = max(lvl_of(A), lvl_of(B)) + 1;
            out = make_int2((int)i, (*gl + 1) << 1);
            *mt = 1;
        }
        break;
    case RV_OP_ADDCONST:
    case RV_OP_SUBCONST:
        out = make_int2(A.x, A.y ^ cb);
        break;
    case RV_OP_MULCONST:
        out = cb ? A : make_int2(-1, 0);
        break;
    case RV_OP_MUL:
        *gl = max(lvl_of(A), lvl_of(B)) + 1;
        out = make_int2((int)i, (*gl + 1) << 1);
        break;
    default:  // AssertZero; a B2A's reconstruction also has a value, its own computed row
        *gl = lvl_of(A) + 1;
        if (op.reserved & PS_OP) {
            out = make_int2((int)i, (*gl + 1) << 1);
            *mt = 1;
        }
        break;
    }
    return out;
}
// ... and at lazy_k = RV_LIN_K, lazy_slack = 1, balance = 0 (a forced compile): a sum of n rows read f times stays symbolic while
// f x (n - 1) extra operand rows cost no more than the n reads and one write of materialising it
__device__ inline uint4 value_lazy(const rv_op& op, uint32_t i, int2 p, const uint32_t* uses, const uint4* V3, const int* glvl, int* gl, uint32_t* mt) {
    const uint4 A = form_of(V3, p.x), B = form_of(V3, p.y);
    const uint32_t cb = (uint32_t)(op.imm & 1);
    const uint4 none = make_uint4(0, 0, 0, 0);
    uint4 out = none;
    switch (op.opcode) {
    case RV_OP_INPUT:
    case RV_OP_RANDOM:
        *gl = 0;
        out = make_uint4(i, 0, 0, 1);
        break;
    case RV_OP_CONST:
        out = make_uint4(0, 0, 0, cb << 2);
        break;
    case RV_OP_ADD:
    case RV_OP_SUB: {
        uint32_t rows[2 * RV_LIN_K];
        const uint32_t n = (uint32_t)form_xor(A, B, rows), c = form_c(A) ^ form_c(B);
        const uint32_t f = uses[i];
        if (f == 0) break;  // an unread sum is dropped
        if (n <= 1 || (n <= (uint32_t)RV_LIN_K && (uint64_t)f * (n - 1) <= (uint64_t)n + 1)) {
            out = make_uint4(rows[0], rows[1], rows[2], n | c << 2);
        } else {  // one G_XORK of n rows; the constant goes into the gate
            int l = -1;
#pragma unroll
            for (int k = 0; k < 2 * RV_LIN_K; k++)
                if ((uint32_t)k < n) l = max(l, glvl[rows[k] & ~ROW_COMP]);
            *gl = l + 1;
            *mt = 1;
            out = make_uint4(i | ROW_COMP, 0, 0, 1u | n << 8);
        }
        break;
    }
    case RV_OP_ADDCONST:
    case RV_OP_SUBCONST:
        out = make_uint4(A.x, A.y, A.z, (A.w & 7u) ^ cb << 2);
        break;
    case RV_OP_MULCONST:
        out = cb ? make_uint4(A.x, A.y, A.z, A.w & 7u) : none;
        break;
    case RV_OP_MUL:
        *gl = max(form_lvl(A, glvl), form_lvl(B, glvl)) + 1;
        out = make_uint4(i, 0, 0, 1);
        break;
    default:  // AssertZero; a B2A's reconstruction also has a value, its own computed row
        *gl = form_lvl(A, glvl) + 1;
        if (op.reserved & PS_OP) {
            out = make_uint4(i | ROW_COMP, 0, 0, 1);
            *mt = 1;
        }
        break;
    }
    return out;
}

// a Z64 op's level (run_pass, case RV_DOM_Z64): Input, Random and Const 0, every other gate one above its deepest operand; SSA 0 and
// a chunk's carried slots (p < 0) count as -1
// (a B2A: one above its deepest reconstruction, which k_z_b2a_levels wrote before the rounds)
__device__ inline int level_z64(const rv_op& op, uint32_t i, int2 p, const int* glvl) {
    if (op.opcode == ZOP_B2A) return glvl[i];
    if (op_reads(op.opcode) == 0) return 0;
    return max(p.x >= 0 ? glvl[p.x] : -1, p.y >= 0 ? glvl[p.y] : -1) + 1;
}

// step 3: one round.  rounds[r] = {first frontier slot, count}; the ops whose last pending operand this round resolves form
// round r + 1's frontier.  FORM_LAZY: the values are lazy sums in V3 (V unused); FORM_K1: one row or a constant in V (V3 unused);
// FORM_Z64: Z64 ops, which have a level and no value (V, V3, mat unused).
enum { FORM_K1 = 0, FORM_LAZY = 1, FORM_Z64 = 2 };
template <int FORM>
__global__ __launch_bounds__(TB) void k_cd_round(uint32_t r, uint32_t chunk, const rv_op* ops, const int2* prod, const uint32_t* uses, const uint32_t* cons_off,
                                                 const uint32_t* cons, uint32_t* rem, int2* V, uint4* V3, int* glvl, uint32_t* mat, uint32_t* frontier,
                                                 uint2* rounds) {
    // the next frontier is gathered in LDS and appended with one global atomic per workgroup (65 536 appends to one counter per
    // round of the benchmark circuit otherwise); what does not fit the LDS queue is appended one by one
    constexpr uint32_t FQ = 2048;
    __shared__ uint32_t q[FQ];
    __shared__ uint32_t qn, qbase;
    if (threadIdx.x == 0) qn = 0;
    __syncthreads();
    const uint2 R = rounds[r];
    const uint32_t nb = R.x + R.y;
    if (blockIdx.x == 0 && threadIdx.x == 0) rounds[r + 1].x = nb;
    for (uint32_t t = blockIdx.x * TB + threadIdx.x; t < R.y; t += gridDim.x * TB) {
        const uint32_t i = frontier[R.x + t];
        const rv_op op = ops[i];
        const int2 p = prod[i];
        int gl = -1;
        uint32_t mt = 0;
        if constexpr (FORM == FORM_Z64) gl = level_z64(op, i, p, glvl);
        else if constexpr (FORM == FORM_LAZY) V3[i] = value_lazy(op, i, p, uses, V3, glvl, &gl, &mt);
        else V[i] = value_k1(op, i, p, chunk, uses, V, &gl, &mt);
        glvl[i] = gl;
        if constexpr (FORM != FORM_Z64) mat[i] = mt;
        const uint32_t c0 = cons_off[i], c1 = cons_off[i + 1];  // (not c0 + uses[i]: k_cd_live adds the reads after the program to uses)
        for (uint32_t k = c0; k < c1; k++) {
            const uint32_t c = cons[k];
            if (atomicSub(&rem[c], 1u) == 1u) {
                const uint32_t s = atomicAdd(&qn, 1u);
                if (s < FQ) q[s] = c;
                else frontier[nb + atomicAdd(&rounds[r + 1].y, 1u)] = c;
            }
        }
    }
    __syncthreads();
    const uint32_t m = min(qn, FQ);
    if (threadIdx.x == 0 && m) qbase = atomicAdd(&rounds[r + 1].y, m);
    __syncthreads();
    for (uint32_t j = threadIdx.x; j < m; j += TB) frontier[nb + qbase + j] = q[j];
}

struct DevStats {
    int max_level;
    uint32_t n_gates, n_mat, pad;
    unsigned long long operand_rows;
};
// the gate count, materialised XORs, levels and operand rows (one atomic per workgroup and counter)
template <bool LAZY>
__global__ __launch_bounds__(TB) void k_cd_stats(const rv_op* ops, size_t n, const int2* prod, const int2* V, const uint4* V3, const int* glvl,
                                                 const uint32_t* mat, DevStats* st) {
    __shared__ int sl[TB];
    __shared__ uint32_t sg[TB], sm[TB], so[TB];
    const size_t i = (size_t)blockIdx.x * TB + threadIdx.x;
    int l = -1;
    uint32_t g = 0, m = 0, o = 0;
    if (i < n) {
        l = glvl[i];
        g = l >= 0;
        m = mat[i];
        const uint32_t opc = ops[i].opcode;
        const int2 p = prod[i];
        if constexpr (LAZY) {  // the rows of the operand forms; a materialised sum's own
            if (opc == RV_OP_MUL) o = form_n(form_of(V3, p.x)) + form_n(form_of(V3, p.y));
            else if (opc == RV_OP_ASSERTZERO) o = form_n(form_of(V3, p.x));
            else if (m) o = V3[i].w >> 8;
        } else {
            if (opc == RV_OP_MUL) o = is_row(val_of(V, p.x)) + is_row(val_of(V, p.y));
            else if (opc == RV_OP_ASSERTZERO) o = is_row(val_of(V, p.x));
            else if (m) o = 2;
        }
    }
    sl[threadIdx.x] = l, sg[threadIdx.x] = g, sm[threadIdx.x] = m, so[threadIdx.x] = o;
    __syncthreads();
    for (int s = TB / 2; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) {
            sl[threadIdx.x] = max(sl[threadIdx.x], sl[threadIdx.x + s]);
            sg[threadIdx.x] += sg[threadIdx.x + s];
            sm[threadIdx.x] += sm[threadIdx.x + s];
            so[threadIdx.x] += so[threadIdx.x + s];
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        atomicMax(&st->max_level, sl[0]);
        atomicAdd(&st->n_gates, sg[0]);
        atomicAdd(&st->n_mat, sm[0]);
        atomicAdd(&st->operand_rows, (unsigned long long)so[0]);
    }
}

// step 5: the (level, class) key of every gate (LevelRange classes: Mul of one-base operands 0, other Mul 1, two-row Xor 2,
// any other Xor 3 -- lazy sums only --, the rest 4; ops without a gate get `sentinel`, behind every gate)
template <bool LAZY>
__global__ __launch_bounds__(TB) void k_cd_keys(const rv_op* ops, size_t n, const int2* prod, const int2* V, const uint4* V3, const int* glvl,
                                                const uint32_t* mat, uint32_t sentinel, uint32_t* keys, uint32_t* vals) {
    const size_t i = (size_t)blockIdx.x * TB + threadIdx.x;
    if (i >= n) return;
    const int l = glvl[i];
    uint32_t key = sentinel;
    if (l >= 0) {
        const uint32_t opc = ops[i].opcode;
        uint32_t cls = 4;
        if (opc == RV_OP_MUL) {
            const int2 p = prod[i];
            if constexpr (LAZY) cls = (form_n(form_of(V3, p.x)) == 1 && form_n(form_of(V3, p.y)) == 1) ? 0u : 1u;
            else cls = (is_row(val_of(V, p.x)) && is_row(val_of(V, p.y))) ? 0u : 1u;
        } else if (opc != RV_OP_ASSERTZERO && mat[i]) {  // (a reconstruction has a computed row too: class 4)
            cls = 2;
            if constexpr (LAZY) cls = (V3[i].w >> 8) == 2 ? 2u : 3u;
        }
        key = (uint32_t)l * 5u + cls;
    }
    keys[i] = key;
    vals[i] = (uint32_t)i;
}
// pos[k] = first sorted gate with key >= k, k in [0, n_buckets]
__global__ __launch_bounds__(TB) void k_cd_bounds(const uint32_t* sk, size_t n_gates, uint32_t n_buckets, uint32_t* pos) {
    const size_t p = (size_t)blockIdx.x * TB + threadIdx.x;
    if (p > n_gates) return;
    const uint32_t lo = p == 0 ? 0u : sk[p - 1] + 1u;
    const uint32_t hi = p == n_gates ? n_buckets : sk[p];
    for (uint32_t k = lo; k <= hi; k++) pos[k] = (uint32_t)p;
}

// a value's row as a share row index: a chunk's carried rows, the PRG rows (Input / Random: m, Mul: m + 1), then the computed rows
// (zero row first)
__device__ inline uint32_t row_index(const rv_op* ops, const C4* cx, const uint32_t* comp, const Seeds& s, uint32_t pad, int q) {
    if (q == -1) return s.base + pad;
    if (q < -1) return (uint32_t)(-2 - q);
    const uint32_t opc = ops[q].opcode;
    if (opc == RV_OP_MUL) return s.base + s.m0 + cx[q].m + 1;
    if (opc == RV_OP_INPUT || opc == RV_OP_RANDOM) return s.base + s.m0 + cx[q].m;
    return s.base + pad + 1 + comp[q];
}
// the host compiler sorts a sum's rows as it names them before the final numbering: PRG rows, carried rows, computed rows
__device__ inline uint32_t row_rank(const Seeds& s, uint32_t pad, uint32_t row) { return row < s.base ? 1u : row >= s.base + pad ? 2u : 0u; }
__device__ inline uint32_t wave_max_u32(uint32_t v) {
    for (int s = 32; s > 0; s >>= 1) v = max(v, (uint32_t)__shfl_xor((int)v, s));
    return v;
}
// the gate records in (level, class, program) order, the per-level mask blocks and the online rows' levels
// (pad: the PRG rows, whole cipher blocks; a gate with key >= 4 sits behind the chunk's materialised carried forms)
// LAZY: Builder::fill of whole forms (up to RV_LIN_K rows per operand), a materialised sum of up to 2 RV_LIN_K rows
template <bool LAZY>
__global__ __launch_bounds__(TB) void k_cd_gates(const uint32_t* sk, const uint32_t* sv, size_t n_gates, const rv_op* ops, const int2* prod, const int2* V,
                                                 const uint4* V3, const C4* cx, const uint32_t* comp, Seeds s, uint32_t pad, Gate* gates,
                                                 uint32_t* need_raw, uint32_t* on_lvl) {
    const size_t p = (size_t)blockIdx.x * TB + threadIdx.x;
    const bool valid = p < n_gates;
    uint32_t l = 0, need = 0;
    if (valid) {
        l = sk[p] / 5u;
        const uint32_t i = sv[p];
        const rv_op op = ops[i];
        const C4 c = cx[i];
        const int2 pr = prod[i];
        int2 A = make_int2(-1, 0), B = A;
        uint4 FA = make_uint4(0, 0, 0, 0), FB = FA;
        if constexpr (LAZY) FA = form_of(V3, pr.x), FB = form_of(V3, pr.y);
        else A = val_of(V, pr.x), B = val_of(V, pr.y);
        const uint32_t e = c.in + c.mul + c.as, x = c.mul + c.as;  // e: the online row among the piece's own
        const uint32_t eo = s.on0 + e, m = s.m0 + c.m, zero = s.base + pad;
        Gate g;
        g.dst = s.base, g.m = s.base, g.eo = 0, g.ep = 0, g.x = 0;  // (the host compiler's unused fields: PRG row 0 after the carried rows)
        for (int k = 0; k < RV_LIN_K; k++) g.a[k] = zero, g.b[k] = zero;
        switch (op.opcode) {
        case RV_OP_INPUT:
            g.op = G_INPUT;
            g.m = g.dst = s.base + m;
            g.eo = eo;
            g.x = c.in;
            need = m / 128 + 1;
            on_lvl[e] = l;
            break;
        case RV_OP_RANDOM:
            g.op = G_RANDOM;
            g.m = g.dst = s.base + m;
            need = m / 128 + 1;
            break;
        case RV_OP_MUL: {
            if constexpr (LAZY) {
                const uint32_t na = form_n(FA), nb = form_n(FB);
                g.op = G_MUL | na << 8 | nb << 12 | form_c(FA) << 16 | form_c(FB) << 17;
                for (int k = 0; k < RV_LIN_K; k++) {
                    if ((uint32_t)k < na) g.a[k] = row_index(ops, cx, comp, s, pad, (int)(form_row(FA, k) & ~ROW_COMP));
                    if ((uint32_t)k < nb) g.b[k] = row_index(ops, cx, comp, s, pad, (int)(form_row(FB, k) & ~ROW_COMP));
                }
            } else {
                const uint32_t na = is_row(A), nb = is_row(B);
                g.op = G_MUL | na << 8 | nb << 12 | (uint32_t)(A.y & 1) << 16 | (uint32_t)(B.y & 1) << 17;
                if (na) g.a[0] = row_index(ops, cx, comp, s, pad, A.x);
                if (nb) g.b[0] = row_index(ops, cx, comp, s, pad, B.x);
            }
            g.m = s.base + m;
            g.dst = s.base + m + 1;
            g.eo = eo;
            g.ep = s.pre0 + c.mul;
            g.x = x;
            need = (m + 1) / 128 + 1;
            on_lvl[e] = l;
            break;
        }
        case RV_OP_ASSERTZERO: {
            const uint32_t gop = is_recon(op) ? G_RECON : G_ASSERT;
            if (gop == G_RECON) g.dst = zero + 1 + comp[i];
            if constexpr (LAZY) {
                const uint32_t na = form_n(FA);
                g.op = gop | na << 8 | form_c(FA) << 16;
                for (int k = 0; k < RV_LIN_K; k++)
                    if ((uint32_t)k < na) g.a[k] = row_index(ops, cx, comp, s, pad, (int)(form_row(FA, k) & ~ROW_COMP));
            } else {
                const uint32_t na = is_row(A);
                g.op = gop | na << 8 | (uint32_t)(A.y & 1) << 16;
                if (na) g.a[0] = row_index(ops, cx, comp, s, pad, A.x);
            }
            g.eo = eo;
            g.x = x;
            on_lvl[e] = l;
            break;
        }
        default: {  // a materialised Add / Sub: its two rows in the host compiler's order
            if constexpr (LAZY) {  // (Builder::materialise: the first RV_LIN_K rows in a[], the rest in b[], the constant in the gate)
                uint32_t rows[2 * RV_LIN_K];
                const uint32_t nr = (uint32_t)form_xor(FA, FB, rows), na = min(nr, (uint32_t)RV_LIN_K);
                g.op = G_XORK | na << 8 | (nr - na) << 12 | (form_c(FA) ^ form_c(FB)) << 16;
#pragma unroll
                for (int k = 0; k < RV_LIN_K; k++) {
                    if ((uint32_t)k < nr) g.a[k] = row_index(ops, cx, comp, s, pad, (int)(rows[k] & ~ROW_COMP));
                    if ((uint32_t)(RV_LIN_K + k) < nr) g.b[k] = row_index(ops, cx, comp, s, pad, (int)(rows[RV_LIN_K + k] & ~ROW_COMP));
                }
                g.dst = zero + 1 + comp[i];
                break;
            }
            const uint32_t ra = row_index(ops, cx, comp, s, pad, A.x), rb = row_index(ops, cx, comp, s, pad, B.x);
            const uint32_t ka = row_rank(s, pad, ra), kb = row_rank(s, pad, rb);
            const bool a_first = ka < kb || (ka == kb && ra < rb);
            g.op = G_XORK | 2u << 8 | (uint32_t)((A.y ^ B.y) & 1) << 16;
            g.a[0] = a_first ? ra : rb;
            g.a[1] = a_first ? rb : ra;
            g.dst = zero + 1 + comp[i];
            break;
        }
        }
        gates[p + (sk[p] >= 4u ? s.n_wbmat : 0u)] = g;
    }
    // a wavefront's gates mostly share a level: one atomic for them
    const uint32_t l0 = (uint32_t)__shfl((int)l, 0);
    if (__all(!valid || l == l0)) {
        const uint32_t m = wave_max_u32(need);
        if ((threadIdx.x & 63u) == 0 && m) atomicMax(&need_raw[l0], m);
    } else if (valid && need) {
        atomicMax(&need_raw[l], need);
    }
}
// step 6 (chunk mode).  Per wire: m = the piece wrote it, mul = its final form still reads a carried row (materialised first: two wires
// swapped by a piece must not race), as = the final form has a row (else it is a constant); lastw = the op that wrote it last.
constexpr uint32_t NO_WRITER = 0xFFFFFFFFu;
__global__ __launch_bounds__(TB) void k_cd_wb_flags(const uint32_t* sv, const uint32_t* seg_lo, const uint32_t* seg_hi, uint32_t W, const int2* V, C4* fl,
                                                    uint32_t* lastw) {
    const size_t w = (size_t)blockIdx.x * TB + threadIdx.x;
    if (w >= W) return;
    C4 f{0, 0, 0, 0};
    uint32_t q = NO_WRITER;
    if (seg_hi[w] > seg_lo[w]) {
        q = sv[seg_hi[w] - 1];
        const int2 v = V[q];
        f.m = 1;
        f.mul = v.x < -1;
        f.as = is_row(v);
    }
    fl[w] = f;
    lastw[w] = q;
}
// fx: the exclusive scan of the flags.  The materialised carried forms take the computed rows after the ops' own (n_mat of them) and
// level 0's class 3 (from *pos3; null: the piece has no op gate); the write-backs follow every other gate (from wb_at).
__global__ __launch_bounds__(TB) void k_cd_wb_gates(const uint32_t* lastw, const C4* fx, uint32_t W, const rv_op* ops, const int2* V, const C4* cx,
                                                    const uint32_t* comp, Seeds s, uint32_t pad, uint32_t n_mat, const uint32_t* pos3, uint32_t wb_at,
                                                    Gate* gates) {
    const size_t w = (size_t)blockIdx.x * TB + threadIdx.x;
    if (w >= W) return;
    const uint32_t q = lastw[w];
    if (q == NO_WRITER) return;
    const C4 r = fx[w];
    const int2 v = V[q];
    const uint32_t zero = s.base + pad;
    Gate g;
    g.op = G_XORK, g.dst = 0, g.m = s.base, g.eo = 0, g.ep = 0, g.x = 0;
    for (int k = 0; k < RV_LIN_K; k++) g.a[k] = zero, g.b[k] = zero;
    uint32_t row = zero, n = 0, c = (uint32_t)(v.y & 1);
    if (v.x < -1) {
        g.op = G_XORK | 1u << 8 | c << 16;
        g.a[0] = (uint32_t)(-2 - v.x);
        g.dst = zero + 1 + n_mat + r.mul;
        gates[(pos3 ? *pos3 : 0u) + r.mul] = g;
        row = g.dst, n = 1, c = 0;
    } else if (v.x >= 0) {
        row = row_index(ops, cx, comp, s, pad, v.x), n = 1;
    }
    g.op = G_XORK | n << 8 | c << 16;
    g.a[0] = row;
    g.dst = (uint32_t)w;
    gates[wb_at + r.m] = g;
}
// RV_COMPILE_KEEP_WIRES under RV_COMPILE_DEVICE_KEEP_WIRES (whole programs).  Liveness, Builder::live_out: every written wire's final
// value is read once more after the program -- one read of its last writer per wire (not per distinct value), before the value step,
// so a sum that is a wire's final value is not dropped as unread and the lazy rule has the read in f.  Unlike a chunk the reads are
// still counted: an unread sum that is no wire's final value is dropped.  lastw[w] = wire w's last writer (NO_WRITER: never written),
// taken while the writers sort is in place.
__global__ __launch_bounds__(TB) void k_cd_live(const uint32_t* sv, const uint32_t* seg_lo, const uint32_t* seg_hi, uint32_t W, uint32_t* uses,
                                                uint32_t* lastw) {
    const size_t w = (size_t)blockIdx.x * TB + threadIdx.x;
    if (w >= W) return;
    uint32_t q = NO_WRITER;
    if (seg_hi[w] > seg_lo[w]) {
        q = sv[seg_hi[w] - 1];
        atomicAdd(&uses[q], 1u);
    }
    lastw[w] = q;
}
// The wires' final forms (compile_ops_seq: Compiled::wire_forms), once the rows have their numbers: the last writer's value, its rows
// numbered as a gate's operands are, unused slots the zero row; a never-written wire is the all-zero form
template <bool LAZY>
__global__ __launch_bounds__(TB) void k_cd_wire_forms(const uint32_t* lastw, uint32_t W, const rv_op* ops, const int2* V, const uint4* V3, const C4* cx,
                                                      const uint32_t* comp, Seeds s, uint32_t pad, WireForm* forms) {
    const size_t w = (size_t)blockIdx.x * TB + threadIdx.x;
    if (w >= W) return;
    const uint32_t q = lastw[w];
    WireForm f;
    for (int k = 0; k < RV_LIN_K; k++) f.b[k] = s.base + pad;
    f.c = 0;
    if (q != NO_WRITER) {
        if constexpr (LAZY) {
            const uint4 F = V3[q];
            const uint32_t n = form_n(F);
            for (int k = 0; k < RV_LIN_K; k++)
                if ((uint32_t)k < n) f.b[k] = row_index(ops, cx, comp, s, pad, (int)(form_row(F, k) & ~ROW_COMP));
            f.c = form_c(F);
        } else {
            const int2 v = V[q];
            if (is_row(v)) f.b[0] = row_index(ops, cx, comp, s, pad, v.x);
            f.c = (uint32_t)(v.y & 1);
        }
    }
    forms[w] = f;
}
// level_done_on[l] = online rows e whose prefix maximum of levels is <= l; pm = exclusive prefix maximum of on_lvl (n_on + 1 entries)
__global__ __launch_bounds__(TB) void k_cd_done_on(const uint32_t* pm, const uint32_t* on_lvl, size_t n_on, uint32_t n_levels, uint32_t* done_on) {
    const size_t e = (size_t)blockIdx.x * TB + threadIdx.x;
    if (e > n_on) return;
    const uint32_t lo = pm[e];
    const uint32_t hi = e == n_on ? n_levels : max(pm[e], on_lvl[e]);
    for (uint32_t l = lo; l < hi && l < n_levels; l++) done_on[l] = (uint32_t)e;
}

// step 3's launches: rounds until the frontier is empty, in batches between two looks at the round table.  *n_rounds: rounds launched.
// RV_OK, RV_COMPILE_FALLBACK (the cap: a chain of ops this deep compiles on the host) or RV_E_DEVICE.
int run_rounds(hipStream_t st, int form, uint32_t chunk, const rv_op* ops, size_t n, const Dag& d, int2* V, uint4* V3, int* glvl, uint32_t* mat,
               uint32_t* n_rounds) {
    const uint32_t max_rounds = d.max_rounds, round_blocks = std::min<uint32_t>(blocks(n, TB), 1024);
    uint32_t r = 0, batch = 8;
    for (;;) {
        if (r >= max_rounds) return RV_COMPILE_FALLBACK;
        const uint32_t e = std::min(r + batch, max_rounds);
        for (; r < e; r++) {
#define CD_ROUND(F) k_cd_round<F><<<round_blocks, TB, 0, st>>>(r, chunk, ops, d.prod, d.uses, d.cons_off, d.cons, d.rem, V, V3, glvl, mat, d.frontier, d.rounds)
            if (form == FORM_LAZY) CD_ROUND(FORM_LAZY);
            else if (form == FORM_Z64) CD_ROUND(FORM_Z64);
            else CD_ROUND(FORM_K1);
#undef CD_ROUND
        }
        uint2 nxt;
        if (hipGetLastError() != hipSuccess || hipMemcpyAsync(&nxt, d.rounds + r, sizeof nxt, hipMemcpyDeviceToHost, st) != hipSuccess ||
            hipStreamSynchronize(st) != hipSuccess) {
            (void)hipGetLastError();
            return RV_E_DEVICE;
        }
        if (nxt.y == 0) {
            *n_rounds = r;
            return nxt.x == n ? RV_OK : RV_COMPILE_FALLBACK;  // (every op resolves exactly once; the second cannot happen)
        }
        batch = std::min<uint32_t>(batch * 2, 256);
    }
}

// Gate64::a and Gate64::m2 of every B2A (run_pass: first_out and m2_first, as share rows)
__global__ __launch_bounds__(TB) void k_cd_b2a_rows(const uint32_t* b2a_base, uint32_t n_b2a, const C4* cx, const uint32_t* comp, Seeds s, uint32_t pad,
                                                    uint32_t* rows) {
    const uint32_t j = blockIdx.x * TB + threadIdx.x;
    if (j >= n_b2a) return;
    const uint32_t b = b2a_base[j];
    rows[2 * j] = s.base + pad + 1 + comp[b + B2A_RECON0];
    rows[2 * j + 1] = s.base + s.m0 + cx[b].m;
}

// ---- the host phases ----
// What a mixed list's split tells the GF(2) phases (input only): the ops are the list's GF(2) ops in order, B2A expansions among them
struct Mixed {
    const uint32_t* orig;  // op i's place in the whole list (the AssertZero table)
    size_t n_total;        // ops of the whole list
    // B2A expansions in the list (RV_COMPILE_DEVICE_B2A): where each starts, ascending, and what its Gate64 needs from this compile
    // (b2a_rows[2 j] = its first reconstruction's computed row, [2 j + 1] = its first fresh mask's row)
    uint32_t n_b2a;
    const uint32_t* b2a_base;
    uint32_t* b2a_rows;
};
// the words the host reads back (zeroed once; the kernels get pointers to the members)
struct Gf2Words {
    uint32_t flag;   // k_cd_classify: an op the device path does not take, or an op-list error
    C4 tot;          // the counters' totals
    DevStats stats;  // (max_level starts at 0: max_level + 1 levels when there are gates)
    C4 wb;           // a chunk's write-backs: m = their count, mul = materialised carried forms, as = write-backs that read a row
};
// One GF(2) compile between its two phases (device arrays of the work Scratch, except rec_rows and in_rows, which are the result
// Scratch's when the caller keeps them)
struct Gf2State {
    // the request (the caller: ops, n, mx; gf2_begin: the rest)
    const rv_op* ops;
    size_t n;
    const Mixed* mx;  // null: the list is the caller's own
    size_t z64_wires;
    const ChunkStart* chunk;
    uint32_t W;
    bool lazy;  // the lazy-sum form: whole programs only (a chunk is final at K = 1)
    bool keep;  // RV_COMPILE_KEEP_WIRES: the final values are read after the program, and the wires' forms are a result
    Seeds seeds;
    // device arrays (gf2_levels)
    Gf2Words* d_words;
    C4* cx;
    uint32_t *kbuf[2], *vbuf[2], *rec_rows, *in_rows, *as_rec;
    uint64_t* as_op;
    Dag dag;
    int2* V;     // the ops' values at K = 1 (null: lazy sums) ...
    uint4* V3;   // ... or as lazy sums (null: K = 1)
    int* glvl;   // the level of every op's gate (-1: none)
    uint32_t* mat;
    uint32_t* lastw;        // keep: every wire's last writer (gf2_levels)
    WireForm* wire_forms;   // keep: the wires' final forms (gf2_tables; the result Scratch's when the caller keeps them)
    // host numbers of gf2_levels
    C4 tot;
    uint64_t n_on, n_rec;
    uint32_t n_recon, n_as;  // a B2A's reconstructions count in tot.as (as in info.gf2_asserts); n_as: the AssertZero ops
    uint32_t rounds;         // topological rounds launched
    // host numbers of gf2_tables: what the statistics, the write-back scan and the other domain's levels add up to
    DevStats hs;
    uint32_t n_wb, n_wbmat, n_wbrow;  // a chunk's write-backs, its materialised carried forms, the write-backs that read a row
    uint64_t n_gates_ops, n_gates, n_masks, n_masks_pad, n_comp;  // (n_gates_ops: the ops' gates, without the write-back level's)
    uint32_t n_levels_ops, wb_level, n_levels, n_buckets;
};
constexpr uint64_t LIM = 0xFFFFFFFFull - 512;  // what a 32-bit row, gate or transcript index may reach

// the request of one GF(2) compile: RV_OK, or RV_COMPILE_FALLBACK for what the device path leaves to the host compiler whatever the
// list holds (a Z64 op in the list is what sends a program to the host; the Z64 wire count alone does not)
int gf2_begin(const DevCompileRequest& q, Gf2State& g) {
    const size_t gf2_wires = q.gf2_wires;
    g.z64_wires = q.z64_wires, g.chunk = q.chunk, g.lazy = q.force_lazy_k == RV_LIN_K, g.keep = q.keep_wires;
    // (the wires' final values are kept for whole programs, when the caller set RV_COMPILE_DEVICE_KEEP_WIRES)
    if ((q.keep_wires && (!(q.device_bits & RV_COMPILE_DEVICE_KEEP_WIRES) || g.chunk || q.z64_wires >= (1u << 30))) || (q.force_lazy_k && (!g.lazy || g.chunk)) || getenv("RV_LAZY_K") || (g.n == 0 && !g.chunk && !g.mx) || g.n >= (1u << 28) ||
        gf2_wires >= (1u << 31) || (g.chunk && gf2_wires >= (1u << 30)))  // (a chunk names wire w's carried row -2 - w, below the host compiler's CARRY flag bit)
        return RV_COMPILE_FALLBACK;
    g.W = (uint32_t)gf2_wires;
    g.seeds = Seeds{0, 0, 0, 0, 0, 0};
    if (const ChunkStart* c = g.chunk) {
        if (c->mask_phase >= 128 || c->on0 > LIM || c->pre0 > LIM || g.z64_wires > LIM) return RV_COMPILE_FALLBACK;
        g.seeds = Seeds{1, g.W, c->mask_phase, (uint32_t)c->on0, (uint32_t)c->pre0, 0};
    }
    return RV_OK;
}

// steps 1 - 3: classify, the ordinal tables, the DAG, the values and levels
int gf2_levels(Scratch& S, Scratch& R, LapTimer& T, hipStream_t st, Gf2State& g) {
    const size_t n = g.n;
    const uint32_t W = g.W, gb = blocks(n, TB);
    T.mark(LAP_BEGIN);
    // ---- 1. classify ----
    g.cx = S.get<C4>(n + 1);
    for (int k = 0; k < 2; k++) g.kbuf[k] = S.get<uint32_t>(n);
    for (int k = 0; k < 2; k++) g.vbuf[k] = S.get<uint32_t>(n);
    g.d_words = S.get<Gf2Words>(1);
    CDNEED(g.cx && g.kbuf[0] && g.kbuf[1] && g.vbuf[0] && g.vbuf[1] && g.d_words);
    CDCHK(hipMemsetAsync(g.d_words, 0, sizeof(Gf2Words), st));
    const uint32_t n_b2a = g.mx ? g.mx->n_b2a : 0;
    g.n_recon = 64u * n_b2a;  // (n_b2a x 442 < 2^28)
    k_cd_classify<<<gb, TB, 0, st>>>(g.ops, n, W, n_b2a ? 1u : 0u, g.cx, g.kbuf[0], g.vbuf[0], &g.d_words->flag);
    CDCHK(hipGetLastError());
    CDCHK((scan_excl<C4, SumC4>(S, st, g.cx, g.cx, n, &g.d_words->tot)));
    Gf2Words hw;
    CDCHK(hipMemcpyAsync(&hw, g.d_words, sizeof hw, hipMemcpyDeviceToHost, st));
    CDCHK(hipStreamSynchronize(st));
    if (hw.flag) return RV_COMPILE_FALLBACK;  // an op the device path does not take, or an op-list error: the host compiler reports it
    const C4 tot = g.tot = hw.tot;
    g.n_on = (uint64_t)tot.in + tot.mul + tot.as, g.n_rec = (uint64_t)tot.mul + tot.as;
    if (tot.as < g.n_recon) return RV_E_DEVICE;  // (cannot happen: every expansion has its 64 reconstructions)
    g.n_as = tot.as - g.n_recon;
    g.rec_rows = R.get<uint32_t>(g.n_rec);
    g.in_rows = R.get<uint32_t>(tot.in);
    g.as_rec = S.get<uint32_t>(g.n_as);
    g.as_op = S.get<uint64_t>(g.n_as);
    CDNEED(g.rec_rows && g.in_rows && g.as_rec && g.as_op);
    k_cd_ordinals<<<gb, TB, 0, st>>>(g.ops, n, g.cx, g.seeds.on0, g.rec_rows, g.in_rows, g.as_rec, g.as_op, g.mx ? g.mx->orig : nullptr,
                                     g.mx ? g.mx->b2a_base : nullptr, n_b2a);
    CDCHK(hipGetLastError());
    T.mark(LAP_CLASSIFIED);
    // ---- 2. the last writer of every read ----
    if (const int rc = build_dag(S, st, g.ops, n, W, g.seeds.chunk, g.kbuf, g.vbuf, g.dag)) return rc;
    if (g.keep) {  // the reads after the program, before any value is made
        g.lastw = S.get<uint32_t>(W);
        CDNEED(g.lastw);
        k_cd_live<<<blocks(W, TB), TB, 0, st>>>(g.dag.sv, g.dag.seg_lo, g.dag.seg_hi, W, g.dag.uses, g.lastw);
        CDCHK(hipGetLastError());
    }
    T.mark(LAP_DAG);
    // ---- 3. values and levels, round by round ----
    g.V = g.lazy ? nullptr : S.get<int2>(n);
    g.V3 = g.lazy ? S.get<uint4>(n) : nullptr;
    g.glvl = S.get<int>(n);
    g.mat = S.get<uint32_t>(n + 1);
    CDNEED((g.V || g.V3) && g.glvl && g.mat);
    CDCHK(hipMemsetAsync(g.mat + n, 0, 4, st));
    return run_rounds(st, g.lazy ? FORM_LAZY : FORM_K1, g.lazy ? 0u : g.seeds.chunk, g.ops, n, g.dag, g.V, g.V3, g.glvl, g.mat, &g.rounds);
}

// the host's tables, from the downloads (h_pos[k] = first op gate with key >= k; h_need = the levels' own mask-block maxima)
void gf2_fill(Compiled& cc, const Gf2State& g, const std::vector<uint32_t>& h_pos, const std::vector<uint32_t>& h_need) {
    const C4 tot = g.tot;
    const ChunkStart* chunk = g.chunk;
    const uint64_t W = chunk ? g.W : 0, n_levels = g.n_levels;  // (W: the carried rows in front)
    cc.level_start.assign(n_levels + 1, 0);
    cc.level_range.assign(n_levels, LevelRange{});
    cc.level_need_blocks.assign(n_levels, 0);
    uint32_t need = 0;
    // first gate with key >= k: the ops' gates (h_pos), the materialised carried forms (key 3) and the write-backs (the last level's key 3)
    auto first_at = [&](size_t k) {
        uint64_t v = k <= g.n_buckets ? h_pos[k] : g.n_gates_ops;
        if (k >= 4) v += g.n_wbmat;
        if (g.n_wb && k >= (size_t)g.wb_level * 5 + 4) v += g.n_wb;
        return (uint32_t)v;
    };
    for (uint32_t l = 0; l < n_levels; l++) {
        uint32_t e[6];
        for (int j = 0; j < 6; j++) e[j] = first_at((size_t)l * 5 + j);
        cc.level_start[l] = e[0];
        cc.level_range[l] = LevelRange{e[0], e[1], e[2], e[3], e[4], e[5]};
        need = std::max(need, h_need[l]);
        cc.level_need_blocks[l] = need;
        cc.level_done_on[l] += g.seeds.on0;  // (the carried rows in front are complete before level 0)
    }
    cc.level_start[n_levels] = (uint32_t)g.n_gates;
    cc.level_start64.assign(n_levels + 1, 0);
    const uint64_t randoms = (uint64_t)tot.m - tot.in - 2ull * tot.mul;
    cc.n_ssa = 1 + W + g.n - g.n_as;
    cc.n_masks = g.n_masks, cc.n_masks_pad = g.n_masks_pad;
    cc.n_rows = W + g.n_masks_pad + g.n_comp;
    cc.n_on = (chunk ? chunk->on0 : 0) + g.n_on, cc.n_pre = (chunk ? chunk->pre0 : 0) + tot.mul;
    cc.n_in = tot.in, cc.n_rec = g.n_rec, cc.n_random_or_recon = randoms + g.n_recon;
    cc.n_user_random = randoms - g.n_recon;  // (a B2A's 64 fresh masks are not the user's)
    cc.row_prg_base = W, cc.zero_row = W + g.n_masks_pad;
    if (chunk) {  // (the Z64 side of a GF(2) piece: its carried slots and counters, untouched)
        cc.n_ssa64 = 1 + g.z64_wires, cc.n_masks64 = chunk->mask64_phase;
        cc.on_words64 = chunk->on_words64_0, cc.pre_words64 = chunk->pre_words64_0;
    }
    rv_circuit_info& info = cc.info;
    info.n_ops = g.mx ? g.mx->n_total : g.n;
    info.gf2_inputs = tot.in, info.gf2_muls = tot.mul, info.gf2_asserts = tot.as;
    info.gf2_linear = randoms + (g.hs.n_mat - g.n_recon) + g.n_wbmat + g.n_wb;  // (n_mat: every gate with a computed row, reconstructions too)
    info.gf2_masks = g.n_masks, info.z64_masks = cc.n_masks64, info.levels = g.n_levels;
    info.gf2_operand_rows = g.hs.operand_rows + g.n_wbmat + g.n_wbrow;
    info.gf2_rows_written = (uint64_t)g.hs.n_mat + g.n_wbmat + g.n_wb;
}

// the lazy-sum or the K = 1 instantiation of kernel K
#define CD_FORM(K, grid, ...)                                    \
    if (g.lazy) K<true><<<grid, TB, 0, st>>>(__VA_ARGS__);       \
    else K<false><<<grid, TB, 0, st>>>(__VA_ARGS__)
// steps 4 - 6: the statistics and a chunk's write-back flags, the limits and the lazy_forms_pay decision, computed rows, keys, the
// sort, the gate records, level_done_on, the downloads, `out`.  levels64: levels the other domain's ops take (the level count is the
// deeper domain's, Builder::max_level); wb64: a chunk whose Z64 side has write-back gates (they share the GF(2) write-backs' level).
// *gates_out: the gate array, the result Scratch's.
int gf2_tables(Scratch& S, Scratch& R, LapTimer& T, hipStream_t st, Gf2State& g, uint32_t levels64, bool wb64, Compiled& cc, Gate** gates_out) {
    const size_t n = g.n;
    const uint32_t W = g.W, gb = blocks(n, TB);
    const Dag& d = g.dag;
    const C4 tot = g.tot;
    CD_FORM(k_cd_stats, gb, g.ops, n, d.prod, g.V, g.V3, g.glvl, g.mat, &g.d_words->stats);
    CDCHK(hipGetLastError());
    // ---- 6a. (chunk mode) the wires the piece wrote, while the writers sort is still in place ----
    C4* wfl = nullptr;
    uint32_t* lastw = nullptr;
    if (g.chunk) {
        wfl = S.get<C4>(W);
        lastw = S.get<uint32_t>(W);
        CDNEED(wfl && lastw);
        k_cd_wb_flags<<<blocks(W, TB), TB, 0, st>>>(d.sv, d.seg_lo, d.seg_hi, W, g.V, wfl, lastw);
        CDCHK(hipGetLastError());
        CDCHK((scan_excl<C4, SumC4>(S, st, wfl, wfl, W, &g.d_words->wb)));
    }
    Gf2Words hw;
    CDCHK(hipMemcpyAsync(&hw, g.d_words, sizeof hw, hipMemcpyDeviceToHost, st));
    CDCHK(hipStreamSynchronize(st));
    T.mark(LAP_LEVELS);
    g.hs = hw.stats;
    const uint64_t n_gates_ops = g.n_gates_ops = g.hs.n_gates, n_on = g.n_on;
    g.n_levels_ops = n_gates_ops ? (uint32_t)g.hs.max_level + 1 : 0;
    // the write-back level: one G_XORK per written wire behind every other level; the carried forms it reads are level 0's
    g.n_wb = g.chunk ? hw.wb.m : 0, g.n_wbmat = g.chunk ? hw.wb.mul : 0, g.n_wbrow = g.chunk ? hw.wb.as : 0;
    Seeds seeds = g.seeds;
    seeds.n_wbmat = g.n_wbmat;
    // (a mixed list: the deeper domain's levels count, and either domain's write-backs make the last level)
    g.wb_level = std::max<uint32_t>({g.n_levels_ops, g.n_wbmat ? 1u : 0u, levels64});
    const uint32_t n_levels = g.n_levels = (g.n_wb || wb64) ? g.wb_level + 1 : std::max(g.n_levels_ops, levels64);
    g.n_gates = n_gates_ops + g.n_wbmat + g.n_wb;
    // the K = 1 compile is final unless the circuit is deep and narrow (compile_ops_seq): those go to the host compiler
    // (a chunk is compiled once, at K = 1, whatever its shape; a forced lazy-sum compile is final too)
    if (!g.chunk && !g.lazy && n_levels && lazy_forms_pay(n_levels, g.n_gates)) return RV_COMPILE_FALLBACK;
    g.n_masks = (uint64_t)seeds.m0 + tot.m, g.n_masks_pad = (g.n_masks + 127) / 128 * 128;
    g.n_comp = 1 + (uint64_t)g.hs.n_mat + g.n_wbmat;
    if ((uint64_t)W + g.n_masks_pad + g.n_comp > LIM || g.n_masks_pad / 128 > RV_MAX_CTR_BLOCKS || (uint64_t)n_levels * 5 + 1 >= (1ull << 32) ||
        g.n_comp > LIM / 2 || 1 + (uint64_t)W + n > LIM || (uint64_t)seeds.on0 + n_on > LIM || (uint64_t)seeds.pre0 + tot.mul > LIM)
        return RV_COMPILE_FALLBACK;
    const uint32_t pad = (uint32_t)g.n_masks_pad;
    // ---- 4. computed rows ----
    uint32_t* comp = S.get<uint32_t>(n + 1);
    CDNEED(comp);
    CDCHK((scan_excl<uint32_t, SumU32>(S, st, g.mat, comp, n + 1, nullptr)));
    if (g.mx && g.mx->n_b2a) {
        k_cd_b2a_rows<<<blocks(g.mx->n_b2a, TB), TB, 0, st>>>(g.mx->b2a_base, g.mx->n_b2a, g.cx, comp, seeds, pad, g.mx->b2a_rows);
        CDCHK(hipGetLastError());
    }
    // ---- 5. tables ----
    const uint32_t n_buckets = g.n_buckets = g.n_levels_ops * 5;  // (of the ops' gates: the write-back gates do not go through the sort)
    CD_FORM(k_cd_keys, gb, g.ops, n, d.prod, g.V, g.V3, g.glvl, g.mat, n_buckets, g.kbuf[0], g.vbuf[0]);
    CDCHK(hipGetLastError());
    int which = 0;
    CDCHK(radix_sort(S, st, g.kbuf, g.vbuf, n, bit_len(n_buckets), &which));
    const uint32_t *sk = g.kbuf[which], *sv = g.vbuf[which];
    Gate* gates = *gates_out = R.get<Gate>(g.n_gates);
    uint32_t* pos = S.get<uint32_t>((size_t)n_buckets + 1);
    uint32_t* need_raw = S.get<uint32_t>(n_levels);
    uint32_t* on_lvl = S.get<uint32_t>(n_on + 1);
    uint32_t* pm = S.get<uint32_t>(n_on + 1);
    uint32_t* done_on = S.get<uint32_t>(n_levels);
    CDNEED(gates && pos && need_raw && on_lvl && pm && done_on);
    CDCHK(hipMemsetAsync(need_raw, 0, std::max<size_t>(n_levels, 1) * 4, st));
    CDCHK(hipMemsetAsync(on_lvl + n_on, 0, 4, st));
    k_cd_bounds<<<blocks(n_gates_ops + 1, TB), TB, 0, st>>>(sk, n_gates_ops, n_buckets, pos);
    if (n_gates_ops) {
        CD_FORM(k_cd_gates, blocks(n_gates_ops, TB), sk, sv, n_gates_ops, g.ops, d.prod, g.V, g.V3, g.cx, comp, seeds, pad, gates, need_raw, on_lvl);
    }
    if (g.n_wb)
        k_cd_wb_gates<<<blocks(W, TB), TB, 0, st>>>(lastw, wfl, W, g.ops, g.V, g.cx, comp, seeds, pad, g.hs.n_mat, n_buckets >= 3 ? pos + 3 : nullptr,
                                                    (uint32_t)(n_gates_ops + g.n_wbmat), gates);
    if (g.keep && W) {
        g.wire_forms = R.get<WireForm>(W);
        CDNEED(g.wire_forms);
        CD_FORM(k_cd_wire_forms, blocks(W, TB), g.lastw, W, g.ops, g.V, g.V3, g.cx, comp, seeds, pad, g.wire_forms);
    }
    CDCHK(hipGetLastError());
    CDCHK((scan_excl<uint32_t, MaxU32>(S, st, on_lvl, pm, n_on + 1, nullptr)));
    k_cd_done_on<<<blocks(n_on + 1, TB), TB, 0, st>>>(pm, on_lvl, n_on, n_levels, done_on);
    CDCHK(hipGetLastError());
    T.mark(LAP_TABLES);
    // ---- the host's copy (the planners of circuit_upload read it) ----
    cc = Compiled();
    cc.gates.resize(g.n_gates);
    cc.rec_rows.resize(g.n_rec);
    cc.in_rows.resize(tot.in);
    cc.assert_rec2.resize(g.n_as);
    cc.assert_op2.resize(g.n_as);
    std::vector<uint32_t> h_pos((size_t)n_buckets + 1), h_need(n_levels);
    cc.level_done_on.resize(n_levels);
    CDCHK(fetch(st, cc.gates, gates));
    CDCHK(fetch(st, cc.rec_rows, g.rec_rows));
    CDCHK(fetch(st, cc.in_rows, g.in_rows));
    CDCHK(fetch(st, cc.assert_rec2, g.as_rec));
    CDCHK(fetch(st, cc.assert_op2, g.as_op));
    CDCHK(fetch(st, h_pos, pos));
    CDCHK(fetch(st, h_need, need_raw));
    CDCHK(fetch(st, cc.level_done_on, done_on));
    if (g.keep) cc.wire_forms.resize(W);
    CDCHK(fetch(st, cc.wire_forms, g.wire_forms));
    T.mark(LAP_DOWNLOADED);
    CDCHK(hipStreamSynchronize(st));
    gf2_fill(cc, g, h_pos, h_need);
    return RV_OK;
}
#undef CD_FORM
