// see prune_dev.h
//
// The rule of rv_ops_prune (prune.cpp: a backward sweep) in parallel form, from the device compiler's building blocks
// (compile_dev_prims.inc: the scans, the radix sort, Scratch).  Every per-record decision is prune.h's.  One thread per op where the
// step allows it; plain vector atomics and stores only.  The steps:
//   1. classify   the count in force at every op (an exclusive max-scan of the SizeHint fields), compile_ops' checks (the lowest bad
//                 op's index and code in one 64-bit word: atomicMin), the defining ops per domain.  (compact_dev.hip's step 1 without
//                 the pins; the kernels are copies: the compactor's also count what only it needs.)
//   2. writers    per domain with a defining op: the defining ops sorted by destination (stable: by op index within an index).  A
//                 read is resolved by pr_value_read's binary search of the sorted pairs; a B2A resolves its 64 reads the same way.
//                 Resolved reads are not stored: the peeling resolves them again.
//   3. counts     one uint32_t per op: the reads of the value it defines -- one per read by ANY op (two when a and b name the same
//                 value), one per output entry that names the index the value ends on.
//   4. peeling    the first frontier is every defining op that is no root and has count 0.  A round marks each frontier op dropped
//                 and takes one from the count of every value it read; a value that reaches 0 and is no root is appended for the next
//                 round.  One queue of 4 bytes per op (an op enters it at most once), appended to per wavefront (a ballot, one atomic);
//                 the round's bounds live in device words.  A frontier of at most PRUNE_SOLO_LIMIT ops is peeled round after round by
//                 ONE workgroup inside one launch (k_pr_solo: a barrier per layer) until it is empty or outgrows the limit; a wider
//                 one takes a grid-stride launch (k_pr_wide).  In the solo kernel every thread carries the bounds and the layer count
//                 in registers and reads the tail between two barriers: no thread-dependent branch stands around a barrier.  The host
//                 launches PRUNE_LOOK_INTERVAL pairs of the two and then looks at the words.  Layers are counted on the device; after RV_PRUNE_MAX_ROUNDS of them the call falls back to the host.
//   5. emit       the keep flags' exclusive sum; one workgroup per tile of 256 INPUT records gathers its kept records into an LDS
//                 image at the position modulo 16 their bytes have in d_out and writes it in 16-byte stores with an 8-byte piece at an
//                 unfilled end (link_dev.hip's layout), d_old_index beside it; the class counts by a ballot per wavefront, one LDS
//                 atomic per wavefront, one global atomic per workgroup.  The count-only call runs the counts alone.
// The host reads device words after step 1, inside the peeling loop (the first look comes before any round: a list with nothing dead
// launches none) and at the end.
#include "prune_dev.h"

#include <stdlib.h>

#include <algorithm>
#include <atomic>
#include <vector>

namespace rv {
namespace {
#include "compile_dev_prims.inc"
static_assert(TB == (int)PRUNE_WG && TB == (int)PRUNE_TILE, "the sizes rv_hook_prune_limits reports");
static_assert(PRUNE_SOLO_LIMIT % PRUNE_WG == 0, "the solo kernel walks its frontier in whole strides");

// the words of one call in device memory
enum { S_ERR_LO, S_ERR_HI, S_HINT_Z, S_HINT_G, S_DEF_G, S_DEF_Z, S_Q_LO, S_Q_HI, S_Q_TAIL, S_ROUNDS, S_WIDE_DONE, S_CLS, S_WORDS = S_CLS + PR_CLASSES };

std::atomic<uint64_t> g_launches[4];  // emit, count-only, peeling, fall-backs

// the two domains' sorted (index, op) pairs; nd: the defining ops of the domain (the pairs behind them carry the key W)
struct Writers {
    const uint32_t *sk[2], *sv[2];
    uint32_t nd[2];
};

// ---- step 1 ----
__global__ __launch_bounds__(TB) void k_pr_hints(const rv_op* ops, size_t n, uint32_t* hz, uint32_t* hg) {
    const size_t i = (size_t)blockIdx.x * TB + threadIdx.x;
    if (i >= n) return;
    const bool h = ops[i].domain == RV_DOM_SIZEHINT;
    hz[i] = h ? ops[i].a : 0u;
    hg[i] = h ? ops[i].b : 0u;
}
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
__global__ __launch_bounds__(TB) void k_pr_outputs(const uint32_t* outs, size_t n_outs, int d, Writers w, uint32_t* cnt) {
    const size_t k = (size_t)blockIdx.x * TB + threadIdx.x;
    if (k >= n_outs) return;
    const uint32_t v = pr_value_read(w.sk[d], w.sv[d], w.nd[d], outs[k], PR_NONE);
    if (v != PR_NONE) atomicAdd(&cnt[v], 1u);
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

// ---- step 5 ----
template <bool EMIT>
__global__ __launch_bounds__(TB) void k_pr_emit(const rv_op* ops, size_t n, const uint32_t* cnt, const uint32_t* keep, const uint32_t* pos, uint32_t* state,
                                                uint8_t* out, uint32_t* old_index) {
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
            if (old_index) old_index[at] = (uint32_t)i;
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

void fill_info(rv_prune_info* info, size_t n, size_t n_kept, const uint32_t* cls, uint32_t rounds, uint32_t on_device) {
    if (!info) return;
    *info = rv_prune_info{};
    info->n_kept = n_kept, info->n_dropped = n - n_kept;
    uint64_t* c = &info->dropped_gf2_mul;  // (the nine class counters lie in prune.h's order)
    for (int k = 0; k < PR_CLASSES; k++) c[k] = cls[k];
    info->device_rounds = rounds, info->on_device = on_device;
}

// the fall-back: the list copied down, the host sweep, the result uploaded
int prune_on_host(Scratch& S, hipStream_t st, const rv_op* d_ops, size_t n, uint64_t z64_wires, uint64_t gf2_wires, const uint32_t* const outs[2],
                  const size_t n_outs[2], rv_op* d_out, size_t cap, size_t* n_out, uint32_t* d_old_index, rv_prune_info* info, uint32_t rounds) {
    g_launches[3]++;
    std::vector<rv_op> h(n);
    std::vector<uint32_t> old(d_out && d_old_index ? n : 0);
    CDCHK(hipMemcpyAsync(h.data(), d_ops, n * sizeof(rv_op), hipMemcpyDeviceToHost, st));
    CDCHK(hipStreamSynchronize(st));
    size_t kept = 0;
    rv_prune_info pi;
    // (in place on the host copy; the capacity is judged here against the caller's)
    if (const int rc = rv_ops_prune(h.data(), n, z64_wires, gf2_wires, outs[0], n_outs[0], outs[1], n_outs[1], nullptr, 0, &kept, nullptr, &pi)) return rc;
    if (d_out) {
        if (cap < kept) return RV_E_ARG;
        if (const int rc = rv_ops_prune(h.data(), n, z64_wires, gf2_wires, outs[0], n_outs[0], outs[1], n_outs[1], h.data(), n, &kept,
                                        old.empty() ? nullptr : old.data(), &pi))
            return rc;
        if (kept) CDCHK(hipMemcpyAsync(d_out, h.data(), kept * sizeof(rv_op), hipMemcpyHostToDevice, st));
        if (kept && d_old_index) CDCHK(hipMemcpyAsync(d_old_index, old.data(), kept * sizeof(uint32_t), hipMemcpyHostToDevice, st));
        CDCHK(hipStreamSynchronize(st));
    }
    if (n_out) *n_out = kept;
    if (info) {
        *info = pi;
        info->device_rounds = rounds, info->on_device = 0;
    }
    return RV_OK;
}

int prune_impl(hipStream_t st, const DevAlloc& A, const rv_op* ops, size_t n, uint64_t z64_wires, uint64_t gf2_wires, const uint32_t* const outs[2],
               const size_t n_outs[2], rv_op* d_out, size_t cap, size_t* n_out, uint32_t* d_old_index, rv_prune_info* info) {
    Scratch S(A, st);
    const uint32_t gb = blocks(n, TB);
    const uint32_t max_rounds = prune_max_rounds();
    uint32_t* state = S.get<uint32_t>(S_WORDS);
    uint32_t *kbuf[2][2] = {}, *vbuf[2][2] = {};
    for (int k = 0; k < 2; k++) kbuf[0][k] = S.get<uint32_t>(n), vbuf[0][k] = S.get<uint32_t>(n);
    CDNEED(state && kbuf[0][0] && kbuf[0][1] && vbuf[0][0] && vbuf[0][1]);
    std::vector<uint32_t> h(S_WORDS);

    // step 1 (the hints and their scans borrow the first sort's buffers)
    CDCHK(hipMemsetAsync(state, 0, S_WORDS * 4, st));
    CDCHK(hipMemsetAsync(state, 0xFF, 8, st));
    k_pr_hints<<<gb, TB, 0, st>>>(ops, n, kbuf[0][0], kbuf[0][1]);
    CDCHK((scan_excl<uint32_t, MaxU32>(S, st, kbuf[0][0], vbuf[0][0], n, &state[S_HINT_Z])));
    CDCHK((scan_excl<uint32_t, MaxU32>(S, st, kbuf[0][1], vbuf[0][1], n, &state[S_HINT_G])));
    k_pr_classify<<<gb, TB, 0, st>>>(ops, n, z64_wires, gf2_wires, vbuf[0][0], vbuf[0][1], state);
    CDCHK(hipGetLastError());
    CDCHK(fetch(st, h, state));
    CDCHK(hipStreamSynchronize(st));
    if (h[S_ERR_HI] != 0xFFFFFFFFu || h[S_ERR_LO] != 0xFFFFFFFFu) return (int)(h[S_ERR_LO] & 0xFFu);
    const uint64_t W[2] = {std::max<uint64_t>(gf2_wires, h[S_HINT_G]), std::max<uint64_t>(z64_wires, h[S_HINT_Z])};
    if (W[PR_G] >= (1ull << 31) || W[PR_Z] >= (1ull << 31)) return RV_E_UNSUPPORTED;
    for (int d = 0; d < 2; d++)
        for (size_t k = 0; k < n_outs[d]; k++)
            if (outs[d][k] >= W[d]) return RV_E_ARG;

    // step 2
    Writers w = {};
    int set = 0;  // the buffers the next sort takes
    for (int d = 0; d < 2; d++) {
        w.nd[d] = h[S_DEF_G + d];
        if (!w.nd[d]) continue;  // (every read of the domain finds no value: the search looks at no pair)
        if (set == 1) {
            for (int k = 0; k < 2; k++) kbuf[1][k] = S.get<uint32_t>(n), vbuf[1][k] = S.get<uint32_t>(n);
            CDNEED(kbuf[1][0] && kbuf[1][1] && vbuf[1][0] && vbuf[1][1]);
        }
        k_pr_keys<<<gb, TB, 0, st>>>(ops, n, d, (uint32_t)W[d], kbuf[set][0], vbuf[set][0]);
        int which = 0;
        CDCHK(radix_sort(S, st, kbuf[set], vbuf[set], n, bit_len(W[d]), &which));
        w.sk[d] = kbuf[set][which], w.sv[d] = vbuf[set][which];
        set++;
    }

    // step 3
    uint32_t *cnt = S.get<uint32_t>(n), *keep = S.get<uint32_t>(n), *queue = S.get<uint32_t>(n);
    CDNEED(cnt && keep && queue);
    CDCHK(hipMemsetAsync(cnt, 0, n * 4, st));
    k_pr_count<<<gb, TB, 0, st>>>(ops, n, w, cnt, keep);
    for (int d = 0; d < 2; d++) {
        if (!n_outs[d] || !w.nd[d]) continue;
        uint32_t* d_outs = S.get<uint32_t>(n_outs[d]);
        CDNEED(d_outs);
        CDCHK(hipMemcpyAsync(d_outs, outs[d], n_outs[d] * 4, hipMemcpyHostToDevice, st));
        k_pr_outputs<<<blocks(n_outs[d], TB), TB, 0, st>>>(d_outs, n_outs[d], d, w, cnt);
    }

    // step 4
    k_pr_frontier<<<gb, TB, 0, st>>>(ops, n, cnt, queue, state);
    k_pr_begin<<<1, 64, 0, st>>>(state);
    CDCHK(hipGetLastError());
    for (;;) {
        CDCHK(fetch(st, h, state));
        CDCHK(hipStreamSynchronize(st));
        if (!h[S_WIDE_DONE]) {
            if (h[S_Q_HI] == h[S_Q_LO]) break;
            if (h[S_ROUNDS] >= max_rounds)
                return prune_on_host(S, st, ops, n, z64_wires, gf2_wires, outs, n_outs, d_out, cap, n_out, d_old_index, info, h[S_ROUNDS]);
        }
        for (uint32_t k = 0; k < PRUNE_LOOK_INTERVAL; k++) {
            k_pr_solo<<<1, TB, 0, st>>>(ops, (uint32_t)n, w, cnt, keep, queue, state, max_rounds);
            k_pr_wide<<<std::min<uint32_t>(PRUNE_WIDE_BLOCKS, gb), TB, 0, st>>>(ops, (uint32_t)n, w, cnt, keep, queue, state, max_rounds);
            g_launches[2] += 2;
        }
        CDCHK(hipGetLastError());
    }
    // (every dropped op entered the queue once, and nothing else did)
    const size_t n_kept = n - h[S_Q_TAIL];
    const uint32_t rounds = h[S_ROUNDS];

    // step 5
    if (d_out) {
        if (cap < n_kept) return RV_E_ARG;
        uint32_t* pos = S.get<uint32_t>(n);
        CDNEED(pos);
        CDCHK((scan_excl<uint32_t, SumU32>(S, st, keep, pos, n, nullptr)));
        k_pr_emit<true><<<gb, TB, 0, st>>>(ops, n, cnt, keep, pos, state, reinterpret_cast<uint8_t*>(d_out), d_old_index);
        g_launches[0]++;
    } else {
        k_pr_emit<false><<<gb, TB, 0, st>>>(ops, n, cnt, keep, nullptr, state, nullptr, nullptr);
        g_launches[1]++;
    }
    CDCHK(hipGetLastError());
    CDCHK(fetch(st, h, state));
    CDCHK(hipStreamSynchronize(st));
    if (n_out) *n_out = n_kept;
    fill_info(info, n, n_kept, &h[S_CLS], rounds, 1);
    return RV_OK;
}
#undef CDCHK
#undef CDNEED
}  // namespace

uint32_t prune_max_rounds() {
    const char* e = getenv("RV_PRUNE_MAX_ROUNDS");
    if (!e || !*e) return PRUNE_MAX_ROUNDS_DEFAULT;
    char* end = nullptr;
    const unsigned long long v = strtoull(e, &end, 10);
    return (*end || v == 0 || v > 0xFFFFFFFFull) ? PRUNE_MAX_ROUNDS_DEFAULT : (uint32_t)v;
}

void prune_launches(uint64_t out[4]) {
    for (int k = 0; k < 4; k++) out[k] = g_launches[k].load();
}

int prune_ops_device(hipStream_t st, const DevAlloc& A, const rv_op* d_ops, size_t n_ops, uint64_t z64_wires, uint64_t gf2_wires,
                     const uint32_t* const outs[2], const size_t n_outs[2], rv_op* d_out, size_t cap, size_t* n_out, uint32_t* d_old_index,
                     rv_prune_info* info) {
    if (n_ops >= (1ull << 31)) return RV_E_UNSUPPORTED;
    if (n_ops == 0) {  // (no launch; the outputs are still judged against the stated counts)
        const uint64_t W[2] = {gf2_wires, z64_wires};
        for (int d = 0; d < 2; d++)
            for (size_t k = 0; k < n_outs[d]; k++)
                if (outs[d][k] >= W[d]) return RV_E_ARG;
        if (n_out) *n_out = 0;
        if (info) {
            *info = rv_prune_info{};
            info->on_device = 1;
        }
        return RV_OK;
    }
    return prune_impl(st, A, d_ops, n_ops, z64_wires, gf2_wires, outs, n_outs, d_out, cap, n_out, d_old_index, info);
}

}  // namespace rv
