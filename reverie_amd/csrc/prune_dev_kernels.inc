// The pruning kernels that the whole-list call (prune_dev.hip) and the windowed one (prune_win.hip) both launch: steps 1 - 4 of
// DESIGN §23.3 and the emit.  #included inside an anonymous namespace of namespace rv, behind compile_dev_prims.inc (TB, the scans,
// the sort), prune.h and win_stage.h (step 1 joins a windowed stage's digest), as compile_dev_prims.inc itself is shared: one text, a
// copy of the code per translation unit.  Every per-record decision is prune.h's.  One thread per op where the step allows it; plain
// vector atomics and stores only.  Steps 1 and 2 have their host halves here too (pr_step1, pr_step2): prune_dev.hip, fold_dev.hip,
// prune_win.hip and fold_win.hip all begin with them.

// the words of one call (the windowed form: of one feed) in device memory
enum { S_ERR_LO, S_ERR_HI, S_HINT_Z, S_HINT_G, S_DEF_G, S_DEF_Z, S_Q_LO, S_Q_HI, S_Q_TAIL, S_ROUNDS, S_WIDE_DONE, S_CLS, S_WORDS = S_CLS + PR_CLASSES };

// the two domains' sorted (index, op) pairs; nd: the defining ops of the domain (the pairs behind them carry the key W)
struct Writers {
    const uint32_t *sk[2], *sv[2];
    uint32_t nd[2];
};

// ---- step 1 ----
// (k_pr_hints is compile_dev_prims.inc's: the compactors launch it too)
__global__ __launch_bounds__(TB) void k_pr_classify(const rv_op* ops, size_t n, uint64_t decl_z, uint64_t decl_g, const uint32_t* cz, const uint32_t* cg,
                                                    uint32_t* state) {
    __shared__ uint32_t cnt[2];
    if (threadIdx.x < 2) cnt[threadIdx.x] = 0;
    __syncthreads();
    const size_t i = (size_t)blockIdx.x * TB + threadIdx.x;
    int d = -1;
    if (i < n) {
        const rv_op op = ops[i];
        const uint64_t nz = decl_z > cz[i] ? decl_z : cz[i], ng = decl_g > cg[i] ? decl_g : cg[i];
        const int rc = pr_check(op, nz, ng);
        if (rc != RV_OK) atomicMin((unsigned long long*)state, ((unsigned long long)i << 8) | (unsigned long long)rc);
        else d = pr_def(op);
    }
    for (int k = 0; k < 2; k++) {
        const unsigned long long m = __ballot(d == k);
        if ((threadIdx.x & 63u) == 0 && m) atomicAdd(&cnt[k], (uint32_t)__popcll(m));
    }
    __syncthreads();
    if (threadIdx.x < 2 && cnt[threadIdx.x]) atomicAdd(&state[S_DEF_G + threadIdx.x], cnt[threadIdx.x]);
}

// ---- step 2 ----
__global__ __launch_bounds__(TB) void k_pr_keys(const rv_op* ops, size_t n, int d, uint32_t W, uint32_t* key, uint32_t* idx) {
    const size_t i = (size_t)blockIdx.x * TB + threadIdx.x;
    if (i >= n) return;
    const rv_op op = ops[i];
    key[i] = pr_def(op) == d ? op.dst : W;
    idx[i] = (uint32_t)i;
}

// ---- steps 1 and 2 on the host (S: the call's Scratch; the caller took `state` and the buffers from it) ----
// Step 1 of ops [0, n) on `st`, with `in` ([PR_G], [PR_Z]) the counts in force before ops[0]: the n_words words of `state` cleared,
// the hints (hint[0], hint[1]: Z64, GF(2)), their exclusive max-scans (into scan[0], scan[1]), the classify kernel, the words fetched
// into h.  hint == nullptr: the ops are judged against `in` alone -- no hint of theirs raises a count; scan[0] is zeroed and stands
// for both scans.  win: the feed of a windowed stage, whose digest the ops join (win->sum: their sum); nullptr: a whole list.
// -> RV_OK and W = the counts in force behind the last op; the lowest bad op's code; RV_E_UNSUPPORTED for a count of 2^31; or
// RV_E_NOMEM / RV_E_DEVICE.  The stream is idle afterwards.
int pr_step1(Scratch& S, hipStream_t st, const rv_op* ops, size_t n, uint32_t* state, size_t n_words, const uint64_t in[2], uint32_t* const* hint,
             uint32_t* const scan[2], WinFeed* win, std::vector<uint32_t>& h, uint64_t W[2]) {
    const uint32_t gb = blocks(n, TB);
    CDCHK(hipMemsetAsync(state, 0, n_words * 4, st));
    CDCHK(hipMemsetAsync(state, 0xFF, 8, st));
    if (win) CDCHK(stage_digest(win->stage, ops, n, win->first));
    if (hint) {
        k_pr_hints<<<gb, TB, 0, st>>>(ops, n, hint[0], hint[1]);
        CDCHK((scan_excl<uint32_t, MaxU32>(S, st, hint[0], scan[0], n, &state[S_HINT_Z])));
        CDCHK((scan_excl<uint32_t, MaxU32>(S, st, hint[1], scan[1], n, &state[S_HINT_G])));
    } else {
        CDCHK(hipMemsetAsync(scan[0], 0, n * 4, st));
    }
    k_pr_classify<<<gb, TB, 0, st>>>(ops, n, in[PR_Z], in[PR_G], scan[0], scan[hint ? 1 : 0], state);
    CDCHK(hipGetLastError());
    CDCHK(fetch(st, h, state));
    if (win) CDCHK(stage_fetch_digest(win->stage, &win->sum));
    CDCHK(hipStreamSynchronize(st));
    if (h[S_ERR_HI] != 0xFFFFFFFFu || h[S_ERR_LO] != 0xFFFFFFFFu) return (int)(h[S_ERR_LO] & 0xFFu);
    W[PR_G] = std::max<uint64_t>(in[PR_G], h[S_HINT_G]), W[PR_Z] = std::max<uint64_t>(in[PR_Z], h[S_HINT_Z]);
    return (W[PR_G] >= (1ull << 31) || W[PR_Z] >= (1ull << 31)) ? RV_E_UNSUPPORTED : RV_OK;
}
// Step 2: per domain with a defining op (h: step 1's words) the keys and the sort, into w.  kbuf[0], vbuf[0]: the caller's first
// set of buffers (step 1 may have borrowed them); the second set is taken from S only when both domains define.
int pr_step2(Scratch& S, hipStream_t st, const rv_op* ops, size_t n, const uint64_t W[2], const std::vector<uint32_t>& h, uint32_t* kbuf[2][2],
             uint32_t* vbuf[2][2], Writers* w) {
    const uint32_t gb = blocks(n, TB);
    *w = Writers{};
    int set = 0;  // the buffers the next sort takes
    for (int d = 0; d < 2; d++) {
        w->nd[d] = h[S_DEF_G + d];
        if (!w->nd[d]) continue;  // (every read of the domain finds no value: the search looks at no pair)
        if (set == 1) {
            for (int k = 0; k < 2; k++) kbuf[1][k] = S.get<uint32_t>(n), vbuf[1][k] = S.get<uint32_t>(n);
            CDNEED(kbuf[1][0] && kbuf[1][1] && vbuf[1][0] && vbuf[1][1]);
        }
        k_pr_keys<<<gb, TB, 0, st>>>(ops, n, d, (uint32_t)W[d], kbuf[set][0], vbuf[set][0]);
        int which = 0;
        CDCHK(radix_sort(S, st, kbuf[set], vbuf[set], n, bit_len(W[d]), &which));
        w->sk[d] = kbuf[set][which], w->sv[d] = vbuf[set][which];
        set++;
    }
    return RV_OK;
}

// ---- step 3 ----
// (also sets the keep flags: every op is kept until a round drops it)
__global__ __launch_bounds__(TB) void k_pr_count(const rv_op* ops, size_t n, Writers w, uint32_t* cnt, uint32_t* keep) {
    const size_t i = (size_t)blockIdx.x * TB + threadIdx.x;
    if (i >= n) return;
    keep[i] = 1u;
    const rv_op op = ops[i];
    const uint32_t r = pr_n_reads(op);
    const int rd = pr_read_dom(op);
    for (uint32_t k = 0; k < r; k++) {
        const uint32_t v = pr_value_read(w.sk[rd], w.sv[rd], w.nd[rd], pr_read(op, k), (uint32_t)i);
        if (v != PR_NONE) atomicAdd(&cnt[v], 1u);
    }
}

// ---- step 4 ----
// `mine` (at most one op per lane) appended to the queue: one atomic per wavefront.  Every lane of the wavefront calls it.  (An op
// enters the queue at most once, so a place is below `cap`, the list's length; the test keeps a wrong count from becoming a store
// outside the queue.)
__device__ inline void q_append(bool have, uint32_t op_index, uint32_t* queue, uint32_t cap, uint32_t* state) {
    const unsigned long long m = __ballot(have);
    if (!m) return;  // (the same in every lane)
    const uint32_t lane = threadIdx.x & 63u, leader = (uint32_t)__ffsll((long long)m) - 1u;
    uint32_t base = 0;
    if (lane == leader) base = atomicAdd(&state[S_Q_TAIL], (uint32_t)__popcll(m));
    base = __shfl(base, (int)leader);
    const uint32_t at = base + (uint32_t)__popcll(m & ((1ull << lane) - 1ull));
    if (have && at < cap) queue[at] = op_index;
}
__global__ __launch_bounds__(TB) void k_pr_frontier(const rv_op* ops, size_t n, const uint32_t* cnt, uint32_t* queue, uint32_t* state) {
    const size_t i = (size_t)blockIdx.x * TB + threadIdx.x;
    bool dead = false;
    if (i < n) {
        const rv_op op = ops[i];
        dead = pr_def(op) >= 0 && !pr_root(op) && cnt[i] == 0u;
    }
    q_append(dead, (uint32_t)i, queue, (uint32_t)n, state);
}
// the first frontier is the queue so far
__global__ void k_pr_begin(uint32_t* state) {
    if (threadIdx.x == 0 && blockIdx.x == 0) state[S_Q_HI] = state[S_Q_TAIL];
}
// One frontier op (or none: !have) peeled: marked dropped, its reads resolved again and taken from their values' counts, the values
// that reach 0 and are no root appended.  Every lane of the wavefront calls it; the loop runs as long as any lane has a read left.
__device__ inline void peel(bool have, uint32_t i, const rv_op* ops, uint32_t n, const Writers& w, uint32_t* cnt, uint32_t* keep, uint32_t* queue,
                            uint32_t* state) {
    rv_op op = {};
    uint32_t r = 0;
    int rd = 0;
    if (have) {
        op = ops[i];
        keep[i] = 0u;
        r = pr_n_reads(op), rd = pr_read_dom(op);
    }
    for (uint32_t k = 0; __ballot(k < r) != 0ull; k++) {
        bool freed = false;
        uint32_t v = PR_NONE;
        if (k < r) {
            v = pr_value_read(w.sk[rd], w.sv[rd], w.nd[rd], pr_read(op, k), i);
            if (v != PR_NONE && atomicSub(&cnt[v], 1u) == 1u) freed = !pr_root(ops[v]);
        }
        q_append(freed, v, queue, n, state);
    }
}
// a word that is the same in every thread of the workgroup, as a scalar: the loops and branches that go by it stay whole
__device__ inline uint32_t uniform(uint32_t v) { return (uint32_t)__builtin_amdgcn_readfirstlane((int)v); }
// One workgroup: frontiers of at most PRUNE_SOLO_LIMIT ops, layer after layer, until one is empty or wider, or the bound is reached.
// EVERY thread keeps the round's bounds and the layer count in registers, and every thread takes the same way through the loop: no
// branch around a barrier depends on the thread.  (A loop whose bounds thread 0 alone read and wrote, between barriers, was compiled
// into one where the other lanes of thread 0's wavefront went round without it.)  The words go back to device memory at the end,
// every thread storing the same values.
__global__ __launch_bounds__(TB) void k_pr_solo(const rv_op* ops, uint32_t n, Writers w, uint32_t* cnt, uint32_t* keep, uint32_t* queue, uint32_t* state,
                                                uint32_t max_rounds) {
    uint32_t lo = uniform(state[S_Q_LO]), hi = uniform(state[S_Q_HI]), rounds = uniform(state[S_ROUNDS]);
    const uint32_t tail0 = uniform(state[S_Q_TAIL]);
    if (uniform(state[S_WIDE_DONE])) rounds += 1u, lo = hi, hi = tail0;  // the layer a wide launch peeled
    __syncthreads();  // every thread has read the words (the appends below move the tail, the stores at the end the rest)
    while (hi != lo && hi - lo <= PRUNE_SOLO_LIMIT && rounds < max_rounds) {
        for (uint32_t base = lo; base < hi; base += TB) {  // (whole strides: every lane of a wavefront calls peel)
            const uint32_t at = base + threadIdx.x;
            const bool have = at < hi;
            // (the entry may have been written by another wavefront of this launch: read where the stores went)
            const uint32_t i = have ? __hip_atomic_load(&queue[at], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0u;
            peel(have, i, ops, n, w, cnt, keep, queue, state);
        }
        __threadfence();
        __syncthreads();  // the layer's appends are done ...
        const uint32_t tail = uniform(__hip_atomic_load(&state[S_Q_TAIL], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
        __syncthreads();  // ... and every thread has read the tail before the next layer moves it
        rounds += 1u, lo = hi, hi = tail < n ? tail : n;
    }
    state[S_Q_LO] = lo, state[S_Q_HI] = hi, state[S_ROUNDS] = rounds, state[S_WIDE_DONE] = 0u;
}
// a frontier wider than the solo limit, grid-stride; the next solo launch counts the layer and moves the words on
__global__ __launch_bounds__(TB) void k_pr_wide(const rv_op* ops, uint32_t n, Writers w, uint32_t* cnt, uint32_t* keep, uint32_t* queue, uint32_t* state,
                                                uint32_t max_rounds) {
    const uint32_t lo = uniform(state[S_Q_LO]), hi = uniform(state[S_Q_HI]);
    if (hi - lo <= PRUNE_SOLO_LIMIT || uniform(state[S_ROUNDS]) >= max_rounds) return;  // (no launch of this kind changes these words)
    state[S_WIDE_DONE] = 1u;                                                            // (every thread stores the same word)
    const uint64_t stride = (uint64_t)gridDim.x * TB;
    for (uint64_t base = (uint64_t)lo + (uint64_t)blockIdx.x * TB; base < hi; base += stride) {
        const uint64_t at = base + threadIdx.x;
        const bool have = at < hi;
        peel(have, have ? queue[at] : 0u, ops, n, w, cnt, keep, queue, state);
    }
}
// Step 4 on `st`, from the first frontier to an empty one: PRUNE_LOOK_INTERVAL pairs of the two launches, then a look at the words
// (the first look comes before any round: a list with nothing dead launches none).  h: the words as they stand at the end (the stream
// is idle then); *gave_up: max_rounds layers were peeled and the frontier is not empty; *launches: the peeling launches made.
inline hipError_t peel_layers(hipStream_t st, const rv_op* ops, size_t n, const Writers& w, uint32_t* cnt, uint32_t* keep, uint32_t* queue, uint32_t* state,
                              uint32_t max_rounds, std::vector<uint32_t>& h, bool* gave_up, uint64_t* launches) {
    const uint32_t gb = blocks(n, TB);
    *gave_up = false;
    k_pr_frontier<<<gb, TB, 0, st>>>(ops, n, cnt, queue, state);
    k_pr_begin<<<1, 64, 0, st>>>(state);
    hipError_t e = hipGetLastError();
    while (e == hipSuccess) {
        e = fetch(st, h, state);
        if (e == hipSuccess) e = hipStreamSynchronize(st);
        if (e != hipSuccess) break;
        if (!h[S_WIDE_DONE]) {
            if (h[S_Q_HI] == h[S_Q_LO]) break;
            if (h[S_ROUNDS] >= max_rounds) {
                *gave_up = true;
                break;
            }
        }
        for (uint32_t k = 0; k < PRUNE_LOOK_INTERVAL; k++) {
            k_pr_solo<<<1, TB, 0, st>>>(ops, (uint32_t)n, w, cnt, keep, queue, state, max_rounds);
            k_pr_wide<<<std::min<uint32_t>(PRUNE_WIDE_BLOCKS, gb), TB, 0, st>>>(ops, (uint32_t)n, w, cnt, keep, queue, state, max_rounds);
            *launches += 2;
        }
        e = hipGetLastError();
    }
    return e;
}

// ---- step 5 ----
// (old_first: the ordinal of ops[0] in the old list -- 0 for a whole list, the feed's first ordinal for a window)
template <bool EMIT>
__global__ __launch_bounds__(TB) void k_pr_emit(const rv_op* ops, size_t n, const uint32_t* cnt, const uint32_t* keep, const uint32_t* pos, uint32_t* state,
                                                uint8_t* out, uint32_t* old_index, uint32_t old_first) {
    __shared__ __attribute__((aligned(16))) uint8_t raw[EMIT ? PR_IMAGE : 16];
    __shared__ uint32_t s_cls[PR_CLASSES];
    if (threadIdx.x < PR_CLASSES) s_cls[threadIdx.x] = 0;
    __syncthreads();
    const size_t t0 = (size_t)blockIdx.x * TB;
    const uint32_t mine = (uint32_t)std::min<size_t>(TB, n - t0);
    const size_t i = t0 + threadIdx.x;
    int cls = -1;
    bool kept = false;
    rv_op op = {};
    if (threadIdx.x < mine) {
        op = ops[i];
        kept = keep[i] != 0u;
        if (!kept) cls = pr_class(op);
        else if (pr_is_input(op) && cnt[i] == 0u) cls = PR_C_INPUT_G + pr_def(op);
    }
    for (int c = 0; c < PR_CLASSES; c++) {
        const unsigned long long m = __ballot(cls == c);
        if ((threadIdx.x & 63u) == 0 && m) atomicAdd(&s_cls[c], (uint32_t)__popcll(m));
    }
    if (EMIT) {
        // the kept records before the tile, and the tile's own (the same values in every thread)
        const uint32_t first = pos[t0], kept_here = pos[t0 + mine - 1] + keep[t0 + mine - 1] - first;
        const uint32_t sh = pr_image_shift((uint64_t)(uintptr_t)out, first);
        if (kept) {
            const uint32_t at = pos[i];
            const uint64_t* src = reinterpret_cast<const uint64_t*>(&op);
            uint64_t* img = reinterpret_cast<uint64_t*>(raw + sh + (at - first) * 24);
            img[0] = src[0], img[1] = src[1], img[2] = src[2];
            if (old_index) old_index[at] = old_first + (uint32_t)i;
        }
        __syncthreads();
        const uint32_t span = sh + kept_here * 24;
        uint8_t* base = out + (uint64_t)first * 24 - sh;  // 16-byte aligned; only [sh, span) of it is this tile's to write
        for (uint32_t c = threadIdx.x * 16; c < span; c += TB * 16) {
            const uint32_t kind = pr_chunk(c, sh, span);
            if (kind == 3) *reinterpret_cast<uint4*>(base + c) = *reinterpret_cast<const uint4*>(raw + c);
            else if (kind == 1) *reinterpret_cast<uint2*>(base + c) = *reinterpret_cast<const uint2*>(raw + c);
            else if (kind == 2) *reinterpret_cast<uint2*>(base + c + 8) = *reinterpret_cast<const uint2*>(raw + c + 8);
        }
    }
    __syncthreads();
    if (threadIdx.x < PR_CLASSES && s_cls[threadIdx.x]) atomicAdd(&state[S_CLS + threadIdx.x], s_cls[threadIdx.x]);
}
