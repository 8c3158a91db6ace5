// see fold_dev.h
//
// The rule of rv_ops_fold (fold.cpp: a forward sweep) in parallel form, from the device compiler's building blocks
// (compile_dev_prims.inc: the scans, the radix sort, Scratch) and the pruning kernels that fit as they are (prune_dev_kernels.inc:
// the classification, the writers' keys, the queue append).  Every per-record decision is fold.h's.  One thread per op where the
// step allows it; plain vector atomics and stores only.  The steps:
//   1. classify   prune_dev.hip's step 1: the count in force at every op, compile_ops' checks (the lowest bad op's index and code in
//                 one 64-bit word: atomicMin), the defining ops per domain.
//   2. writers    prune_dev.hip's step 2: per domain with a defining op, the defining ops sorted by destination (stable).  A read is
//                 resolved by pr_value_read's binary search of the sorted pairs.
//   3. seed       one thread per op: its reads resolved, the producers of the first two stored (a B2A resolves its 64 again when
//                 they are needed), pending = the reads that have a producer.  A defining op that is known at once (fd_seed: Const, a
//                 zero MulConst, no read with a producer, a Mul with a zero-wire read) sets its state word, stores its value and
//                 enters the queue; its pending is 0.  The kernel also sums pending (the reader pairs of step 4) and notes whether
//                 any read found no producer.  The host looks at the words: no known op and no such read -- the list is copied to
//                 d_out and nothing else is launched; no known op -- straight to step 6.
//   4. readers    the (producer, reader) pairs, one per read with a producer of an op that is not known yet (two when a and b name
//                 one value, up to 64 for a B2A), at the exclusive sum of pending; sorted by producer (stable); off[p] = the first
//                 pair of producer p.  A producer's readers end where the key changes.
//   5. propagate  one queue of 4 bytes per op; an op enters it at most once: whoever makes it known claims its state word with one
//                 compare-and-swap, stores its value and appends it (per wavefront: a ballot, one atomic).  A round takes every op of
//                 the frontier and walks its readers: a Mul reader of a value 0 is claimed as known 0; otherwise one is taken from
//                 the reader's pending, and the thread that brings it to 0 claims the reader and stores fd_eval of its reads' values.
//                 Those values were stored in an earlier round or in step 3, so a launch boundary or the solo kernel's barrier orders
//                 them.  An op is in layer r + 1 exactly if something in layer r made it known: the layer count does not depend on
//                 scheduling.  A frontier of at most FOLD_SOLO_LIMIT ops is stepped layer after layer by ONE workgroup inside one
//                 launch (k_fd_solo: every thread carries the bounds in registers, no thread-dependent branch stands around a
//                 barrier); a wider one takes a grid-stride launch (k_fd_wide).  The host launches FOLD_LOOK_INTERVAL pairs of the
//                 two and then looks at the words.  After RV_FOLD_MAX_ROUNDS layers the call falls back to the host.
//   6. rewrite    one workgroup per tile of 256 records: each thread builds fd_rewrite of its record (from its producers' state words
//                 and values, its own for a B2A) into an LDS image at the position modulo 16 its bytes have in d_out; the image goes
//                 out in 16-byte stores with 8-byte end pieces (pr_chunk).  A tile reads its own records before it writes them and
//                 nothing of another tile's: d_out may be d_ops.  The classes by a ballot per wavefront, one LDS atomic per
//                 wavefront, one global atomic per workgroup.  The count-only call runs the counts alone.
// The host reads device words after step 1, after step 3, inside the propagation loop and at the end.
#include "fold_dev.h"

#include <stdlib.h>

#include <algorithm>
#include <atomic>
#include <vector>

#include "prune_dev.h"

namespace rv {
namespace {
#include "compile_dev_prims.inc"
static_assert(TB == (int)FOLD_WG && TB == (int)FOLD_TILE, "the sizes rv_hook_fold_limits reports");
static_assert(FOLD_SOLO_LIMIT % FOLD_WG == 0, "the solo kernel walks its frontier in whole strides");
#include "prune_dev_kernels.inc"

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

// a value another wavefront may have stored in this launch: read where the stores went
__device__ inline uint64_t ld_val(const uint64_t* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ inline void st_val(uint64_t* p, uint64_t v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// ---- step 3 ----
__global__ __launch_bounds__(TB) void k_fd_seed(const rv_op* ops, size_t n, Writers w, Fold f, uint32_t* queue, uint32_t* state) {
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
        for (uint32_t k = 0; k < r; k++) {
            const uint32_t v = pr_value_read(w.sk[rd], w.sv[rd], w.nd[rd], pr_read(op, k), (uint32_t)i);
            if (v != PR_NONE) have++;
            if (k < 2 && op.domain != RV_DOM_B2A) p[k] = v;
        }
        unwritten = have < r;
        uint64_t value = 0;
        if (pr_def(op) >= 0) {
            if (op.domain == RV_DOM_B2A) {
                known = have == 0;  // (64 zero wires: the value 0)
            } else {
                const bool uw[2] = {r > 0 && p[0] == PR_NONE, r > 1 && p[1] == PR_NONE};
                const uint64_t zero[2] = {0, 0};
                known = fd_seed(op, uw);
                if (known) value = fd_eval(op, zero);
            }
            if (!known) pend = have;
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
// the value of the known record r, all of whose reads are known (their values were stored before this round)
__device__ inline uint64_t value_of(const rv_op& op, uint32_t r, const Writers& w, const Fold& f) {
    if (op.domain == RV_DOM_B2A) {
        uint64_t acc = 0;
        for (uint32_t k = 0; k < 64; k++) {
            const uint32_t p = pr_value_read(w.sk[PR_G], w.sv[PR_G], w.nd[PR_G], op.a + k, r);
            acc |= fd_b2a_bit(k, p == PR_NONE ? 0ull : ld_val(&f.val[p]));
        }
        return acc;
    }
    const uint32_t pa = f.pa[r], pb = f.pb[r];
    const uint64_t v[2] = {pa == PR_NONE ? 0ull : ld_val(&f.val[pa]), pb == PR_NONE ? 0ull : ld_val(&f.val[pb])};
    return fd_eval(op, v);
}
// One frontier op p (or none: !have) told to its readers.  Every lane of the wavefront calls it; the loop runs as long as any lane
// has a reader left.
__device__ inline void spread(bool have, uint32_t p, const rv_op* ops, uint32_t n, const Writers& w, const Fold& f, const Readers& rd, uint32_t* queue,
                              uint32_t* state) {
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
                    value = value_of(op, r, w, f);
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
__global__ __launch_bounds__(TB) void k_fd_solo(const rv_op* ops, uint32_t n, Writers w, Fold f, Readers rd, uint32_t* queue, uint32_t* state,
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
            spread(have && p < n, p, ops, n, w, f, rd, queue, state);
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
__global__ __launch_bounds__(TB) void k_fd_wide(const rv_op* ops, uint32_t n, Writers w, Fold f, Readers rd, uint32_t* queue, uint32_t* state,
                                                uint32_t max_rounds) {
    const uint32_t lo = uniform(state[S_Q_LO]), hi = uniform(state[S_Q_HI]);
    if (hi - lo <= FOLD_SOLO_LIMIT || uniform(state[S_ROUNDS]) >= max_rounds) return;  // (no launch of this kind changes these words)
    state[S_WIDE_DONE] = 1u;                                                           // (every thread stores the same word)
    const uint64_t stride = (uint64_t)gridDim.x * TB;
    for (uint64_t base = (uint64_t)lo + (uint64_t)blockIdx.x * TB; base < hi; base += stride) {
        const uint64_t at = base + threadIdx.x;
        const bool have = at < hi;
        const uint32_t p = have ? queue[at] : 0u;
        spread(have && p < n, p, ops, n, w, f, rd, queue, state);
    }
}

// ---- step 6 ----
template <bool EMIT>
__global__ __launch_bounds__(TB) void k_fd_rewrite(const rv_op* ops, size_t n, Fold f, uint32_t* state, uint8_t* out) {
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
        const uint32_t r = op.domain == RV_DOM_B2A ? 0u : pr_n_reads(op);
        const uint32_t p[2] = {f.pa[i], f.pb[i]};
        bool kn[2] = {false, false};
        uint64_t v[2] = {0, 0};
        for (uint32_t k = 0; k < r; k++) {
            kn[k] = p[k] == PR_NONE || f.known[p[k]] != 0u;
            v[k] = (kn[k] && p[k] != PR_NONE) ? f.val[p[k]] : 0ull;
        }
        const rv_op now = fd_rewrite(op, f.known[i] != 0u, f.val[i], kn, v);
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

std::atomic<uint64_t> g_launches[4];  // rewrite, count-only, propagation, fall-backs

void fill_info(rv_fold_info* info, size_t n, uint64_t n_known, const uint32_t* cls, uint32_t rounds, uint32_t on_device) {
    if (!info) return;
    *info = rv_fold_info{};
    info->n_ops = n, info->n_known = n_known;
    uint64_t* c = &info->gf2_mul_to_const;  // (the nine class counters lie in fold.h's order)
    for (int k = 0; k < FD_CLASSES; k++) c[k] = cls ? cls[k] : 0;
    for (int k = 0; k < FD_REWRITTEN; k++) info->n_rewritten += c[k];
    info->device_rounds = rounds, info->on_device = on_device;
}

// the fall-back: the list copied down, the host sweep, the result uploaded
int fold_on_host(Scratch& S, hipStream_t st, const rv_op* d_ops, size_t n, uint64_t z64_wires, uint64_t gf2_wires, rv_op* d_out, rv_fold_info* info,
                 uint32_t rounds) {
    g_launches[3]++;
    std::vector<rv_op> h(n);
    CDCHK(hipMemcpyAsync(h.data(), d_ops, n * sizeof(rv_op), hipMemcpyDeviceToHost, st));
    CDCHK(hipStreamSynchronize(st));
    rv_fold_info fi;
    if (const int rc = rv_ops_fold(h.data(), n, z64_wires, gf2_wires, d_out ? h.data() : nullptr, &fi)) return rc;
    if (d_out) {
        CDCHK(hipMemcpyAsync(d_out, h.data(), n * sizeof(rv_op), hipMemcpyHostToDevice, st));
        CDCHK(hipStreamSynchronize(st));
    }
    if (info) {
        *info = fi;
        info->device_rounds = rounds, info->on_device = 0;
    }
    return RV_OK;
}

// step 5 on `st`, from the first frontier to an empty one (prune_dev_kernels.inc's peel_layers with this call's kernels; the first
// look was the caller's)
hipError_t propagate(hipStream_t st, const rv_op* ops, size_t n, const Writers& w, const Fold& f, const Readers& rd, uint32_t* queue, uint32_t* state,
                     uint32_t max_rounds, std::vector<uint32_t>& h, bool* gave_up, uint64_t* launches) {
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
            k_fd_solo<<<1, TB, 0, st>>>(ops, (uint32_t)n, w, f, rd, queue, state, max_rounds);
            k_fd_wide<<<std::min<uint32_t>(FOLD_WIDE_BLOCKS, gb), TB, 0, st>>>(ops, (uint32_t)n, w, f, rd, queue, state, max_rounds);
            *launches += 2;
        }
        e = hipGetLastError();
    }
    return e;
}

int fold_impl(hipStream_t st, const DevAlloc& A, const rv_op* ops, size_t n, uint64_t z64_wires, uint64_t gf2_wires, rv_op* d_out, rv_fold_info* info) {
    Scratch S(A, st);
    const uint32_t gb = blocks(n, TB);
    const uint32_t max_rounds = fold_max_rounds();
    uint32_t* state = S.get<uint32_t>(FS_WORDS);
    uint32_t *kbuf[2][2] = {}, *vbuf[2][2] = {};
    for (int k = 0; k < 2; k++) kbuf[0][k] = S.get<uint32_t>(n), vbuf[0][k] = S.get<uint32_t>(n);
    CDNEED(state && kbuf[0][0] && kbuf[0][1] && vbuf[0][0] && vbuf[0][1]);
    std::vector<uint32_t> h(FS_WORDS);

    // step 1 (the hints and their scans borrow the first sort's buffers)
    CDCHK(hipMemsetAsync(state, 0, FS_WORDS * 4, st));
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
    Fold f = {S.get<uint32_t>(n), S.get<uint32_t>(n), S.get<uint32_t>(n), S.get<uint32_t>(n), S.get<uint64_t>(n)};
    uint32_t* queue = S.get<uint32_t>(n);
    CDNEED(f.pa && f.pb && f.pending && f.known && f.val && queue);
    k_fd_seed<<<gb, TB, 0, st>>>(ops, n, w, f, queue, state);
    k_pr_begin<<<1, 64, 0, st>>>(state);
    CDCHK(hipGetLastError());
    CDCHK(fetch(st, h, state));
    CDCHK(hipStreamSynchronize(st));
    if (!h[S_Q_TAIL] && !h[FS_UNWRITTEN]) {  // nothing is known: the list as it is
        if (d_out && d_out != ops) {
            CDCHK(hipMemcpyAsync(d_out, ops, n * sizeof(rv_op), hipMemcpyDeviceToDevice, st));
            CDCHK(hipStreamSynchronize(st));
        }
        fill_info(info, n, 0, nullptr, 0, 1);
        return RV_OK;
    }

    if (h[S_Q_TAIL]) {
        // step 4
        const uint64_t n_pairs = (uint64_t)h[FS_PAIRS] | (uint64_t)h[FS_PAIRS + 1] << 32;
        if (n_pairs >= (1ull << 31)) return fold_on_host(S, st, ops, n, z64_wires, gf2_wires, d_out, info, 0);
        uint32_t* off = S.get<uint32_t>(n);
        uint32_t *pk[2] = {S.get<uint32_t>(n_pairs), S.get<uint32_t>(n_pairs)}, *pv[2] = {S.get<uint32_t>(n_pairs), S.get<uint32_t>(n_pairs)};
        CDNEED(off && pk[0] && pk[1] && pv[0] && pv[1]);
        int which = 0;
        if (n_pairs) {
            CDCHK((scan_excl<uint32_t, SumU32>(S, st, f.pending, off, n, nullptr)));
            k_fd_pairs<<<gb, TB, 0, st>>>(ops, n, w, f, off, (uint32_t)n_pairs, pk[0], pv[0]);
            CDCHK(radix_sort(S, st, pk, pv, n_pairs, bit_len(n), &which));
        }
        CDCHK(hipMemsetAsync(off, 0, n * 4, st));
        if (n_pairs) k_fd_offsets<<<blocks(n_pairs, TB), TB, 0, st>>>(pk[which], (uint32_t)n_pairs, (uint32_t)n, off);
        const Readers rd = {pk[which], pv[which], off, (uint32_t)n_pairs};

        // step 5
        bool gave_up = false;
        uint64_t launches = 0;
        const hipError_t pe = propagate(st, ops, n, w, f, rd, queue, state, max_rounds, h, &gave_up, &launches);
        g_launches[2] += launches;
        CDCHK(pe);
        if (gave_up) return fold_on_host(S, st, ops, n, z64_wires, gf2_wires, d_out, info, h[S_ROUNDS]);
    }
    // (every known op entered the queue once, and nothing else did)
    const uint64_t n_known = h[S_Q_TAIL];
    const uint32_t rounds = h[S_ROUNDS];

    // step 6
    if (d_out) {
        k_fd_rewrite<true><<<gb, TB, 0, st>>>(ops, n, f, state, reinterpret_cast<uint8_t*>(d_out));
        g_launches[0]++;
    } else {
        k_fd_rewrite<false><<<gb, TB, 0, st>>>(ops, n, f, state, nullptr);
        g_launches[1]++;
    }
    CDCHK(hipGetLastError());
    CDCHK(fetch(st, h, state));
    CDCHK(hipStreamSynchronize(st));
    fill_info(info, n, n_known, &h[FS_CLS], rounds, 1);
    return RV_OK;
}
#undef CDCHK
#undef CDNEED
}  // namespace

uint32_t fold_max_rounds() {
    const char* e = getenv("RV_FOLD_MAX_ROUNDS");
    if (!e || !*e) return FOLD_MAX_ROUNDS_DEFAULT;
    char* end = nullptr;
    const unsigned long long v = strtoull(e, &end, 10);
    return (*end || v == 0 || v > 0xFFFFFFFFull) ? FOLD_MAX_ROUNDS_DEFAULT : (uint32_t)v;
}

void fold_launches(uint64_t out[4]) {
    for (int k = 0; k < 4; k++) out[k] = g_launches[k].load();
}

int fold_ops_device(hipStream_t st, const DevAlloc& A, const rv_op* d_ops, size_t n_ops, uint64_t z64_wires, uint64_t gf2_wires, rv_op* d_out,
                    rv_fold_info* info) {
    if (n_ops >= (1ull << 31)) return RV_E_UNSUPPORTED;
    if (n_ops == 0) {  // (no launch)
        if (info) {
            *info = rv_fold_info{};
            info->on_device = 1;
        }
        return RV_OK;
    }
    return fold_impl(st, A, d_ops, n_ops, z64_wires, gf2_wires, d_out, info);
}

}  // namespace rv
