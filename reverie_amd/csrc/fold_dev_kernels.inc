// The folding kernels that the whole-list call (fold_dev.hip) and the windowed one (fold_win.hip) both launch: steps 3 - 6 of
// DESIGN §24.3.  #included inside an anonymous namespace of namespace rv, behind compile_dev_prims.inc (TB, the scans, the sort),
// prune_dev_kernels.inc (the classification, the writers' keys, the queue append) and fold.h, as prune_dev_kernels.inc itself is
// shared: one text, a copy of the code per translation unit.  Every per-record decision is fold.h's.  One thread per op where the
// step allows it; plain vector atomics and stores only.
//
// CARRIED: what a window hears from the ones before it -- one known byte and one value word per index and domain (DESIGN §24.8).  A
// read with no producer in this list is taken from them; with null tables (the whole-list call) it is the zero wire, known 0, and
// every kernel does what it did before there were windows.

// this call's words behind the pruning kernels' (S_ERR_LO .. S_WIDE_DONE are theirs; FS_PAIRS is a 64-bit word)
enum { FS_PAIRS = (S_WORDS + 1) & ~1, FS_UNWRITTEN = FS_PAIRS + 2, FS_CLS, FS_WORDS = FS_CLS + FD_CLASSES };

// the arrays of one call, one entry per op: the producers of reads a and b (PR_NONE: none), the reads whose producer is not known
// yet, the state word (1: known), the value
struct Fold {
    uint32_t *pa, *pb, *pending, *known;
    uint64_t* val;
};
// the reader pairs sorted by producer, and where each producer's begin
struct Readers {
    const uint32_t *rk, *rv, *off;
    uint32_t n_pairs;
};
// the tables as they stand ahead of this list ([PR_G], [PR_Z]; null: none, every index is the zero wire)
struct Carried {
    const uint8_t* K[2];
    const uint64_t* V[2];
};
// a read of index w of domain d that has no producer in this list: is it known, and its value (0 where it is not)
__device__ inline bool carried(const Carried& c, int d, uint32_t w, uint64_t* v) {
    *v = 0;
    if (!c.K[d]) return true;
    if (c.K[d][w] == 0) return false;
    *v = c.V[d][w];
    return true;
}

// a value another wavefront may have stored in this launch: read where the stores went
__device__ inline uint64_t ld_val(const uint64_t* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ inline void st_val(uint64_t* p, uint64_t v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// ---- step 3 ----
// (FS_UNWRITTEN: some read without a producer is known -- with null tables every such read is.  An op with an UNKNOWN read without a
// producer is blocked: its pending may never reach 0.  Nothing but a zero can make it known then, so it keeps no pending at all unless
// it is a Mul with a producer to hear a zero from -- that one counts one read more than it has pairs, and k_fd_pairs fills the place
// with a pair no producer owns.)
__global__ __launch_bounds__(TB) void k_fd_seed(const rv_op* ops, size_t n, Writers w, Fold f, Carried c, uint32_t* queue, uint32_t* state) {
    __shared__ unsigned long long s_pairs;
    __shared__ uint32_t s_unwritten;
    if (threadIdx.x == 0) s_pairs = 0, s_unwritten = 0;
    __syncthreads();
    const size_t i = (size_t)blockIdx.x * TB + threadIdx.x;
    bool known = false, unwritten = false;
    uint32_t pend = 0;
    if (i < n) {
        const rv_op op = ops[i];
        const uint32_t r = pr_n_reads(op);
        const int rd = pr_read_dom(op);
        uint32_t p[2] = {PR_NONE, PR_NONE}, have = 0;
        bool kn[2] = {false, false}, blocked = false;
        uint64_t ev[2] = {0, 0}, bits = 0;
        for (uint32_t k = 0; k < r; k++) {
            const uint32_t v = pr_value_read(w.sk[rd], w.sv[rd], w.nd[rd], pr_read(op, k), (uint32_t)i);
            if (v != PR_NONE) have++;
            if (k < 2 && op.domain != RV_DOM_B2A) p[k] = v;
            if (v == PR_NONE) {
                uint64_t cv;
                const bool ck = carried(c, rd, pr_read(op, k), &cv);
                unwritten = unwritten || ck, blocked = blocked || !ck;
                if (op.domain == RV_DOM_B2A) bits |= fd_b2a_bit(k, cv);
                else if (k < 2) kn[k] = ck, ev[k] = cv;
            }
        }
        uint64_t value = 0;
        if (pr_def(op) >= 0) {
            if (op.domain == RV_DOM_B2A) {
                known = have == 0 && !blocked;  // (64 known bits from ahead of the list; 64 zero wires: the value 0)
                if (known) value = bits;
            } else {
                known = fd_known(op, kn, ev);
                if (known) value = fd_eval(op, ev);
            }
            if (!known) pend = !blocked ? have : (fd_zero_kills(op) && have) ? have + 1u : 0u;
        }
        f.pa[i] = p[0], f.pb[i] = p[1];
        f.pending[i] = pend, f.known[i] = known ? 1u : 0u, f.val[i] = value;
    }
    q_append(known, (uint32_t)i, queue, (uint32_t)n, state);
    unsigned long long sum = pend;
    for (int o = 32; o > 0; o >>= 1) sum += __shfl_down(sum, o);
    const unsigned long long m = __ballot(unwritten);
    if ((threadIdx.x & 63u) == 0) {
        if (sum) atomicAdd(&s_pairs, sum);
        if (m) atomicOr(&s_unwritten, 1u);
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        if (s_pairs) atomicAdd(reinterpret_cast<unsigned long long*>(&state[FS_PAIRS]), s_pairs);
        if (s_unwritten) atomicOr(&state[FS_UNWRITTEN], 1u);
    }
}

// ---- step 4 ----
// (a blocked Mul's last place takes the pair (n, i): n is no producer, the sort puts it behind every producer's pairs)
__global__ __launch_bounds__(TB) void k_fd_pairs(const rv_op* ops, size_t n, Writers w, Fold f, const uint32_t* pos, uint32_t n_pairs, uint32_t* pk,
                                                 uint32_t* pv) {
    const size_t i = (size_t)blockIdx.x * TB + threadIdx.x;
    if (i >= n || f.pending[i] == 0u) return;
    uint32_t at = pos[i];
    const rv_op op = ops[i];
    if (op.domain == RV_DOM_B2A) {
        for (uint32_t k = 0; k < 64; k++) {
            const uint32_t v = pr_value_read(w.sk[PR_G], w.sv[PR_G], w.nd[PR_G], op.a + k, (uint32_t)i);
            if (v != PR_NONE && at < n_pairs) pk[at] = v, pv[at] = (uint32_t)i, at++;
        }
    } else {
        const uint32_t p[2] = {f.pa[i], f.pb[i]};
        for (int k = 0; k < 2; k++)
            if (p[k] != PR_NONE && at < n_pairs) pk[at] = p[k], pv[at] = (uint32_t)i, at++;
        if (at < pos[i] + f.pending[i] && at < n_pairs) pk[at] = (uint32_t)n, pv[at] = (uint32_t)i;
    }
}
// (off is zero before: a producer nobody reads points at pair 0, whose key is another's)
__global__ __launch_bounds__(TB) void k_fd_offsets(const uint32_t* rk, uint32_t n_pairs, uint32_t n, uint32_t* off) {
    const size_t j = (size_t)blockIdx.x * TB + threadIdx.x;
    if (j >= n_pairs) return;
    const uint32_t p = rk[j];
    if ((j == 0 || rk[j - 1] != p) && p < n) off[p] = (uint32_t)j;
}

// ---- step 5 ----
// the value of the known record r, all of whose reads are known (their values were stored before this round, or stand in the tables)
__device__ inline uint64_t value_of(const rv_op& op, uint32_t r, const Writers& w, const Fold& f, const Carried& c) {
    uint64_t cv;
    if (op.domain == RV_DOM_B2A) {
        uint64_t acc = 0;
        for (uint32_t k = 0; k < 64; k++) {
            const uint32_t p = pr_value_read(w.sk[PR_G], w.sv[PR_G], w.nd[PR_G], op.a + k, r);
            acc |= fd_b2a_bit(k, p == PR_NONE ? (carried(c, PR_G, op.a + k, &cv), cv) : ld_val(&f.val[p]));
        }
        return acc;
    }
    const uint32_t pa = f.pa[r], pb = f.pb[r], nr = pr_n_reads(op);
    const int rd = pr_read_dom(op);
    uint64_t v[2] = {0, 0};
    if (nr > 0) v[0] = pa == PR_NONE ? (carried(c, rd, op.a, &cv), cv) : ld_val(&f.val[pa]);
    if (nr > 1) v[1] = pb == PR_NONE ? (carried(c, rd, op.b, &cv), cv) : ld_val(&f.val[pb]);
    return fd_eval(op, v);
}
// One frontier op p (or none: !have) told to its readers.  Every lane of the wavefront calls it; the loop runs as long as any lane
// has a reader left.
__device__ inline void spread(bool have, uint32_t p, const rv_op* ops, uint32_t n, const Writers& w, const Fold& f, const Carried& c, const Readers& rd,
                              uint32_t* queue, uint32_t* state) {
    uint32_t j = 0;
    uint64_t pval = 0;
    if (have) j = rd.off[p], pval = ld_val(&f.val[p]);
    for (;; j++) {
        const bool live = have && j < rd.n_pairs && rd.rk[j] == p;
        if (__ballot(live) == 0ull) break;
        bool claimed = false;
        uint32_t r = 0;
        if (live) {
            r = rd.rv[j];
            if (r < n) {
                const rv_op op = ops[r];
                uint64_t value = 0;
                bool mine = false;
                if (fd_zero_kills(op) && pval == 0) {
                    mine = true;
                } else if (atomicSub(&f.pending[r], 1u) == 1u) {
                    mine = true;
                    value = value_of(op, r, w, f, c);
                }
                if (mine && atomicCAS(&f.known[r], 0u, 1u) == 0u) {
                    st_val(&f.val[r], value);
                    claimed = true;
                }
            }
        }
        q_append(claimed, r, queue, n, state);
    }
}
// One workgroup: frontiers of at most FOLD_SOLO_LIMIT ops, layer after layer, until one is empty or wider, or the bound is reached.
// EVERY thread keeps the round's bounds and the layer count in registers, and every thread takes the same way through the loop: no
// branch around a barrier depends on the thread.  The words go back to device memory at the end, every thread storing the same values.
__global__ __launch_bounds__(TB) void k_fd_solo(const rv_op* ops, uint32_t n, Writers w, Fold f, Carried c, Readers rd, uint32_t* queue, uint32_t* state,
                                                uint32_t max_rounds) {
    uint32_t lo = uniform(state[S_Q_LO]), hi = uniform(state[S_Q_HI]), rounds = uniform(state[S_ROUNDS]);
    const uint32_t tail0 = uniform(state[S_Q_TAIL]);
    if (uniform(state[S_WIDE_DONE])) rounds += 1u, lo = hi, hi = tail0;  // the layer a wide launch stepped
    __syncthreads();  // every thread has read the words (the appends below move the tail, the stores at the end the rest)
    while (hi != lo && hi - lo <= FOLD_SOLO_LIMIT && rounds < max_rounds) {
        for (uint32_t base = lo; base < hi; base += TB) {  // (whole strides: every lane of a wavefront calls spread)
            const uint32_t at = base + threadIdx.x;
            const bool have = at < hi;
            // (the entry may have been written by another wavefront of this launch: read where the stores went)
            const uint32_t p = have ? __hip_atomic_load(&queue[at], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0u;
            spread(have && p < n, p, ops, n, w, f, c, rd, queue, state);
        }
        __threadfence();
        __syncthreads();  // the layer's appends and values are done ...
        const uint32_t tail = uniform(__hip_atomic_load(&state[S_Q_TAIL], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
        __syncthreads();  // ... and every thread has read the tail before the next layer moves it
        rounds += 1u, lo = hi, hi = tail < n ? tail : n;
    }
    state[S_Q_LO] = lo, state[S_Q_HI] = hi, state[S_ROUNDS] = rounds, state[S_WIDE_DONE] = 0u;
}
// a frontier wider than the solo limit, grid-stride; the next solo launch counts the layer and moves the words on
__global__ __launch_bounds__(TB) void k_fd_wide(const rv_op* ops, uint32_t n, Writers w, Fold f, Carried c, Readers rd, uint32_t* queue, uint32_t* state,
                                                uint32_t max_rounds) {
    const uint32_t lo = uniform(state[S_Q_LO]), hi = uniform(state[S_Q_HI]);
    if (hi - lo <= FOLD_SOLO_LIMIT || uniform(state[S_ROUNDS]) >= max_rounds) return;  // (no launch of this kind changes these words)
    state[S_WIDE_DONE] = 1u;                                                           // (every thread stores the same word)
    const uint64_t stride = (uint64_t)gridDim.x * TB;
    for (uint64_t base = (uint64_t)lo + (uint64_t)blockIdx.x * TB; base < hi; base += stride) {
        const uint64_t at = base + threadIdx.x;
        const bool have = at < hi;
        const uint32_t p = have ? queue[at] : 0u;
        spread(have && p < n, p, ops, n, w, f, c, rd, queue, state);
    }
}

// ---- step 6 ----
// record i as the rewrite leaves it (kn, v: its first two reads, as fd_class takes them; not looked at for a B2A)
__device__ inline rv_op rewritten(const rv_op& op, size_t i, const Fold& f, const Carried& c, bool* kn, uint64_t* v) {
    const uint32_t r = op.domain == RV_DOM_B2A ? 0u : pr_n_reads(op);
    const int rd = pr_read_dom(op);
    const uint32_t p[2] = {f.pa[i], f.pb[i]};
    for (uint32_t k = 0; k < r; k++) {
        if (p[k] == PR_NONE) {
            kn[k] = carried(c, rd, pr_read(op, k), &v[k]);
        } else {
            kn[k] = f.known[p[k]] != 0u;
            v[k] = kn[k] ? f.val[p[k]] : 0ull;
        }
    }
    return fd_rewrite(op, f.known[i] != 0u, f.val[i], kn, v);
}
template <bool EMIT>
__global__ __launch_bounds__(TB) void k_fd_rewrite(const rv_op* ops, size_t n, Fold f, Carried cr, uint32_t* state, uint8_t* out) {
    __shared__ __attribute__((aligned(16))) uint8_t raw[EMIT ? PR_IMAGE : 16];
    __shared__ uint32_t s_cls[FD_CLASSES];
    if (threadIdx.x < FD_CLASSES) s_cls[threadIdx.x] = 0;
    __syncthreads();
    const size_t t0 = (size_t)blockIdx.x * TB;
    const uint32_t mine = (uint32_t)std::min<size_t>(TB, n - t0);
    const size_t i = t0 + threadIdx.x;
    const uint32_t sh = EMIT ? pr_image_shift((uint64_t)(uintptr_t)out, t0) : 0u;
    int cls = -1;
    if (threadIdx.x < mine) {
        const rv_op op = ops[i];
        bool kn[2] = {false, false};
        uint64_t v[2] = {0, 0};
        const rv_op now = rewritten(op, i, f, cr, kn, v);
        cls = fd_class(op, now, kn, v);
        if (EMIT) {
            const uint64_t* src = reinterpret_cast<const uint64_t*>(&now);
            uint64_t* img = reinterpret_cast<uint64_t*>(raw + sh + threadIdx.x * 24);
            img[0] = src[0], img[1] = src[1], img[2] = src[2];
        }
    }
    for (int c = 0; c < FD_CLASSES; c++) {
        const unsigned long long m = __ballot(cls == c);
        if ((threadIdx.x & 63u) == 0 && m) atomicAdd(&s_cls[c], (uint32_t)__popcll(m));
    }
    __syncthreads();  // the image is whole, and every record of the tile has been read
    if (EMIT) {
        const uint32_t span = sh + mine * 24;
        uint8_t* base = out + (uint64_t)t0 * 24 - sh;  // 16-byte aligned; only [sh, span) of it is this tile's to write
        for (uint32_t c = threadIdx.x * 16; c < span; c += TB * 16) {
            const uint32_t kind = pr_chunk(c, sh, span);
            if (kind == 3) *reinterpret_cast<uint4*>(base + c) = *reinterpret_cast<const uint4*>(raw + c);
            else if (kind == 1) *reinterpret_cast<uint2*>(base + c) = *reinterpret_cast<const uint2*>(raw + c);
            else if (kind == 2) *reinterpret_cast<uint2*>(base + c + 8) = *reinterpret_cast<const uint2*>(raw + c + 8);
        }
    }
    if (threadIdx.x < FD_CLASSES && s_cls[threadIdx.x]) atomicAdd(&state[FS_CLS + threadIdx.x], s_cls[threadIdx.x]);
}

// step 5 on `st`, from the first frontier to an empty one (prune_dev_kernels.inc's peel_layers with this call's kernels; the first
// look was the caller's)
inline hipError_t propagate(hipStream_t st, const rv_op* ops, size_t n, const Writers& w, const Fold& f, const Carried& c, const Readers& rd, uint32_t* queue,
                            uint32_t* state, uint32_t max_rounds, std::vector<uint32_t>& h, bool* gave_up, uint64_t* launches) {
    const uint32_t gb = blocks(n, TB);
    *gave_up = false;
    hipError_t e = hipSuccess;
    for (bool first = true; e == hipSuccess; first = false) {
        if (!first) {
            e = fetch(st, h, state);
            if (e == hipSuccess) e = hipStreamSynchronize(st);
            if (e != hipSuccess) break;
        }
        if (!h[S_WIDE_DONE]) {
            if (h[S_Q_HI] == h[S_Q_LO]) break;
            if (h[S_ROUNDS] >= max_rounds) {
                *gave_up = true;
                break;
            }
        }
        for (uint32_t k = 0; k < FOLD_LOOK_INTERVAL; k++) {
            k_fd_solo<<<1, TB, 0, st>>>(ops, (uint32_t)n, w, f, c, rd, queue, state, max_rounds);
            k_fd_wide<<<std::min<uint32_t>(FOLD_WIDE_BLOCKS, gb), TB, 0, st>>>(ops, (uint32_t)n, w, f, c, rd, queue, state, max_rounds);
            *launches += 2;
        }
        e = hipGetLastError();
    }
    return e;
}
