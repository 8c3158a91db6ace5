// see prune_dev.h
//
// The rule of rv_ops_prune (prune.cpp: a backward sweep) in parallel form, from the device compiler's building blocks
// (compile_dev_prims.inc: the scans, the radix sort, Scratch).  Every per-record decision is prune.h's.  One thread per op where the
// step allows it; plain vector atomics and stores only.  The kernels are prune_dev_kernels.inc's (prune_win.hip launches the same
// ones on a window); this file holds the whole-list call.  The steps:
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

#include "win_stage.h"

namespace rv {
namespace {
#include "compile_dev_prims.inc"
static_assert(TB == (int)PRUNE_WG && TB == (int)PRUNE_TILE, "the sizes rv_hook_prune_limits reports");
static_assert(PRUNE_SOLO_LIMIT % PRUNE_WG == 0, "the solo kernel walks its frontier in whole strides");
#include "prune_dev_kernels.inc"

// step 3's other half, the whole list's alone (a window hears of the outputs through its needed bytes): one count per output entry
__global__ __launch_bounds__(TB) void k_pr_outputs(const uint32_t* outs, size_t n_outs, int d, Writers w, uint32_t* cnt) {
    const size_t k = (size_t)blockIdx.x * TB + threadIdx.x;
    if (k >= n_outs) return;
    const uint32_t v = pr_value_read(w.sk[d], w.sv[d], w.nd[d], outs[k], PR_NONE);
    if (v != PR_NONE) atomicAdd(&cnt[v], 1u);
}

std::atomic<uint64_t> g_launches[4];  // emit, count-only, peeling, fall-backs

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
    const uint64_t stated[2] = {gf2_wires, z64_wires};
    uint64_t W[2];
    if (const int rc = pr_step1(S, st, ops, n, state, S_WORDS, stated, kbuf[0], vbuf[0], nullptr, h, W)) return rc;
    for (int d = 0; d < 2; d++)
        for (size_t k = 0; k < n_outs[d]; k++)
            if (outs[d][k] >= W[d]) return RV_E_ARG;

    // step 2
    Writers w;
    if (const int rc = pr_step2(S, st, ops, n, W, h, kbuf, vbuf, &w)) return rc;

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
    bool gave_up = false;
    uint64_t launches = 0;
    const hipError_t pe = peel_layers(st, ops, n, w, cnt, keep, queue, state, max_rounds, h, &gave_up, &launches);
    g_launches[2] += launches;
    CDCHK(pe);
    if (gave_up) return prune_on_host(S, st, ops, n, z64_wires, gf2_wires, outs, n_outs, d_out, cap, n_out, d_old_index, info, h[S_ROUNDS]);
    // (every dropped op entered the queue once, and nothing else did)
    const size_t n_kept = n - h[S_Q_TAIL];
    const uint32_t rounds = h[S_ROUNDS];

    // step 5
    if (d_out) {
        if (cap < n_kept) return RV_E_ARG;
        uint32_t* pos = S.get<uint32_t>(n);
        CDNEED(pos);
        CDCHK((scan_excl<uint32_t, SumU32>(S, st, keep, pos, n, nullptr)));
        k_pr_emit<true><<<gb, TB, 0, st>>>(ops, n, cnt, keep, pos, state, reinterpret_cast<uint8_t*>(d_out), d_old_index, 0u);
        g_launches[0]++;
    } else {
        k_pr_emit<false><<<gb, TB, 0, st>>>(ops, n, cnt, keep, nullptr, state, nullptr, nullptr, 0u);
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
