// see prune_win.h
//
// prune_dev.hip's rule for a list that arrives in feeds.  Pruning is a backward data-flow problem: the marks are made
// from the last window to the first, and what a window hears from the ones behind it is one needed byte per wire index and domain.
// The kernels of steps 1 - 4 and the emit are prune_dev_kernels.inc's, launched on the feed as they are launched on a whole list;
// the window step's own decisions (live-out, kill, gen) are prune.h's.  Three passes:
//
// Scan (forwards).  prune_dev.hip's step 1 with the counts in force carried from feed to feed as the classify kernel's seed, and
// the position-keyed digest of the feed (piece_sums.hip, as compact_win.hip sums it).  Nothing is written.  At the end the length,
// the final counts and the digest are fixed; the needed bytes (final counts) and one mark byte per op are taken, and the needed
// bytes of the caller's output indices set.
//
// Mark (backwards; a feed's ops in list order).  Every record is checked against the FINAL counts first (the classify kernel again:
// a record of the scanned list passes, since no count in force exceeds the final one; one that fails addresses nothing).  Then
// steps 2 - 4 on the feed, with
//   live-out   after the reader counts: one thread per sorted pair; the last pair of a key run whose needed byte is set adds one to
//              its op's count (the value is read behind the window);
//   kill       after the peeling: the same run-last threads store 0 to the needed byte (every index the window writes);
//   gen        a launch of its own after kill, one thread per op: a kept op resolves its reads again and stores 1 for each one that
//              escapes the window.  Racing stores to one byte carry the same value;
//   marks      marks[first + i] = keep[i].
// The class counts come from k_pr_emit<false> on the feed and are summed on the host.  A feed whose peeling reaches
// RV_PRUNE_MAX_ROUNDS layers is copied down with the two tables (the kernels have not touched them yet), stepped by prune.h's host
// sweep, and its marks and tables uploaded.
//
// Emit (forwards, any number of times).  The feed's marks widened to words, their exclusive sum, k_pr_emit<true> with the feed's
// first ordinal added to old_index.
#include "prune_win.h"

#include <stdlib.h>

#include <algorithm>
#include <vector>

#include "prune_dev.h"
#include "win_stage.h"

namespace rv {
namespace {
#include "compile_dev_prims.inc"
static_assert(TB == (int)PRUNE_WG && TB == (int)PRUNE_TILE, "the kernels of prune_dev_kernels.inc are launched with TB threads");
#include "prune_dev_kernels.inc"

// ---- scan_end: the needed bytes of the output indices ----
__global__ __launch_bounds__(TB) void k_pw_outputs(const uint32_t* outs, size_t n_outs, uint8_t* N, uint64_t W) {
    const size_t k = (size_t)blockIdx.x * TB + threadIdx.x;
    if (k < n_outs && outs[k] < W) N[outs[k]] = 1;
}

// ---- mark feed ----
// one thread per sorted pair of a domain's defining ops
__global__ __launch_bounds__(TB) void k_pw_live_out(const uint32_t* sk, const uint32_t* sv, uint32_t nd, const uint8_t* N, uint64_t W, uint32_t* cnt) {
    const size_t j = (size_t)blockIdx.x * TB + threadIdx.x;
    if (j < nd && pr_live_out(sk, nd, (uint32_t)j, N, W)) atomicAdd(&cnt[sv[j]], 1u);
}
__global__ __launch_bounds__(TB) void k_pw_kill(const uint32_t* sk, uint32_t nd, uint8_t* N, uint64_t W) {
    const size_t j = (size_t)blockIdx.x * TB + threadIdx.x;
    if (j < nd) pr_kill(sk, nd, (uint32_t)j, N, W);
}
// one thread per op (Ng, Nz: the two needed tables; Wg, Wz: their lengths)
__global__ __launch_bounds__(TB) void k_pw_gen(const rv_op* ops, size_t n, Writers w, const uint32_t* keep, uint8_t* Ng, uint8_t* Nz, uint64_t Wg,
                                               uint64_t Wz) {
    const size_t i = (size_t)blockIdx.x * TB + threadIdx.x;
    if (i < n && keep[i] != 0u) {
        const rv_op op = ops[i];
        const uint32_t r = pr_n_reads(op);
        const int rd = pr_read_dom(op);
        uint8_t* N = rd == PR_G ? Ng : Nz;
        const uint64_t W = rd == PR_G ? Wg : Wz;
        for (uint32_t k = 0; k < r; k++) pr_gen(op, (uint32_t)i, k, w.sk[rd], w.sv[rd], w.nd[rd], N, W);
    }
}
__global__ __launch_bounds__(TB) void k_pw_marks_out(const uint32_t* keep, size_t n, uint8_t* marks) {
    const size_t i = (size_t)blockIdx.x * TB + threadIdx.x;
    if (i < n) marks[i] = keep[i] != 0u ? 1 : 0;
}

// ---- emit feed ----
__global__ __launch_bounds__(TB) void k_pw_marks_in(const uint8_t* marks, size_t n, uint32_t* keep) {
    const size_t i = (size_t)blockIdx.x * TB + threadIdx.x;
    if (i < n) keep[i] = marks[i] != 0 ? 1u : 0u;
}

}  // namespace

enum class Phase { SCAN, MARK, FEED };

struct WinPruner : WinStage {
    Phase phase = Phase::SCAN;
    uint64_t W[2] = {0, 0};  // counts in force ([PR_G], [PR_Z]); final from scan_end on
    std::vector<uint32_t> outs[2];
    uint8_t* need[2] = {nullptr, nullptr};  // W[d] bytes
    uint8_t* marks = nullptr;               // total bytes
    uint64_t n_kept = 0, cls[PR_CLASSES] = {}, rounds = 0, mark_feeds = 0, host_feeds = 0;

    bool at(Phase ph) const { return !failed && phase == ph; }
    size_t state_bytes() const {
        return WIN_BLOCK_BYTES + (need[PR_G] ? (size_t)W[PR_G] : 0) + (need[PR_Z] ? (size_t)W[PR_Z] : 0) + (marks ? (size_t)total : 0);
    }
};

namespace {

int scan_impl(WinPruner* p, const DevAlloc& CA, const rv_op* ops, size_t n) {
    hipStream_t st = p->st;
    Scratch S(CA, st);
    uint32_t* state = S.get<uint32_t>(S_WORDS);
    uint32_t *hint[2] = {S.get<uint32_t>(n), S.get<uint32_t>(n)}, *scan[2] = {S.get<uint32_t>(n), S.get<uint32_t>(n)};
    CDNEED(state && hint[0] && hint[1] && scan[0] && scan[1]);
    std::vector<uint32_t> h(S_WORDS);
    uint64_t W[2];
    WinFeed feed = {*p, p->pos};
    if (const int rc = pr_step1(S, st, ops, n, state, S_WORDS, p->W, hint, scan, &feed, h, W)) {
        p->failed = true;
        return rc;
    }
    p->W[PR_G] = W[PR_G], p->W[PR_Z] = W[PR_Z];
    p->digest += feed.sum;
    p->pos += n;
    return RV_OK;
}

int scan_end_impl(WinPruner* p, const DevAlloc& CA) {
    hipStream_t st = p->st;
    for (int d = 0; d < 2; d++)
        for (uint32_t w : p->outs[d])
            if (w >= p->W[d]) {
                p->failed = true;
                return RV_E_ARG;
            }
    Scratch S(CA, st);
    for (int d = 0; d < 2; d++) {
        p->need[d] = (uint8_t*)p->take((size_t)p->W[d]);
        CDNEED(p->need[d]);
        if (p->W[d]) CDCHK(hipMemsetAsync(p->need[d], 0, (size_t)p->W[d], st));
    }
    p->marks = (uint8_t*)p->take((size_t)p->pos);
    CDNEED(p->marks);
    if (p->pos) CDCHK(hipMemsetAsync(p->marks, 0, (size_t)p->pos, st));
    for (int d = 0; d < 2; d++) {
        const size_t k = p->outs[d].size();
        if (!k) continue;
        uint32_t* d_outs = S.get<uint32_t>(k);
        CDNEED(d_outs);
        CDCHK(hipMemcpyAsync(d_outs, p->outs[d].data(), k * 4, hipMemcpyHostToDevice, st));
        k_pw_outputs<<<blocks(k, TB), TB, 0, st>>>(d_outs, k, p->need[d], p->W[d]);
    }
    CDCHK(hipGetLastError());
    CDCHK(hipStreamSynchronize(st));
    p->total = p->pos, p->digest0 = p->digest;
    p->digest = 0;  // (pos stays at the list's length: the mark pass runs down from it)
    p->phase = Phase::MARK;
    return RV_OK;
}

// the fall-back of one mark feed: the feed and the two tables copied down, the host sweep, the marks and the tables uploaded
int mark_on_host(WinPruner* p, const rv_op* ops, size_t n, uint64_t first, uint64_t cls[PR_CLASSES], uint64_t* kept) {
    hipStream_t st = p->st;
    std::vector<rv_op> h(n);
    std::vector<uint8_t> tab[2] = {std::vector<uint8_t>((size_t)p->W[PR_G]), std::vector<uint8_t>((size_t)p->W[PR_Z])}, keep(n);
    hipError_t e = hipMemcpyAsync(h.data(), ops, n * sizeof(rv_op), hipMemcpyDeviceToHost, st);
    for (int d = 0; d < 2; d++)
        if (e == hipSuccess && p->W[d]) e = hipMemcpyAsync(tab[d].data(), p->need[d], (size_t)p->W[d], hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e == hipSuccess) {
        PrDense need[2] = {{tab[PR_G].data()}, {tab[PR_Z].data()}};
        *kept = pr_window_sweep(h.data(), n, need, keep.data(), cls);
        e = hipMemcpyAsync(p->marks + first, keep.data(), n, hipMemcpyHostToDevice, st);
    }
    for (int d = 0; d < 2; d++)
        if (e == hipSuccess && p->W[d]) e = hipMemcpyAsync(p->need[d], tab[d].data(), (size_t)p->W[d], hipMemcpyHostToDevice, st);
    const hipError_t es = hipStreamSynchronize(st);  // (also after an error: the vectors go while nothing reads them)
    if (e != hipSuccess || es != hipSuccess) {
        (void)hipGetLastError();
        return RV_E_DEVICE;
    }
    return RV_OK;
}

int mark_impl(WinPruner* p, const DevAlloc& CA, const rv_op* ops, size_t n, size_t* n_kept_here) {
    hipStream_t st = p->st;
    Scratch S(CA, st);
    const uint32_t gb = blocks(n, TB);
    const uint32_t max_rounds = prune_max_rounds();
    const uint64_t first = p->pos - n;
    uint32_t* state = S.get<uint32_t>(S_WORDS);
    uint32_t *kbuf[2][2] = {}, *vbuf[2][2] = {};
    for (int k = 0; k < 2; k++) kbuf[0][k] = S.get<uint32_t>(n), vbuf[0][k] = S.get<uint32_t>(n);
    CDNEED(state && kbuf[0][0] && kbuf[0][1] && vbuf[0][0] && vbuf[0][1]);
    std::vector<uint32_t> h(S_WORDS);
    uint64_t W[2];
    WinFeed feed = {*p, first};

    // every record against the final counts (no hint of the feed can raise them)
    if (const int rc = pr_step1(S, st, ops, n, state, S_WORDS, p->W, nullptr, kbuf[0], &feed, h, W))
        return (rc == RV_E_NOMEM || rc == RV_E_DEVICE) ? rc : RV_E_ARG;  // (not the scanned list; nothing was addressed)

    // step 2
    Writers w;
    if (const int rc = pr_step2(S, st, ops, n, p->W, h, kbuf, vbuf, &w)) return rc;

    // step 3, and the live-out
    uint32_t *cnt = S.get<uint32_t>(n), *keep = S.get<uint32_t>(n), *queue = S.get<uint32_t>(n);
    CDNEED(cnt && keep && queue);
    CDCHK(hipMemsetAsync(cnt, 0, n * 4, st));
    k_pr_count<<<gb, TB, 0, st>>>(ops, n, w, cnt, keep);
    for (int d = 0; d < 2; d++)
        if (w.nd[d]) k_pw_live_out<<<blocks(w.nd[d], TB), TB, 0, st>>>(w.sk[d], w.sv[d], w.nd[d], p->need[d], p->W[d], cnt);

    // step 4
    bool gave_up = false;
    uint64_t launches = 0;
    CDCHK(peel_layers(st, ops, n, w, cnt, keep, queue, state, max_rounds, h, &gave_up, &launches));
    uint64_t cls[PR_CLASSES] = {}, kept = 0;
    if (gave_up) {
        if (const int rc = mark_on_host(p, ops, n, first, cls, &kept)) return rc;
        p->host_feeds++;
    } else {
        // (every dropped op entered the queue once, and nothing else did)
        kept = n - h[S_Q_TAIL];
        for (int d = 0; d < 2; d++)
            if (w.nd[d]) k_pw_kill<<<blocks(w.nd[d], TB), TB, 0, st>>>(w.sk[d], w.nd[d], p->need[d], p->W[d]);
        k_pw_gen<<<gb, TB, 0, st>>>(ops, n, w, keep, p->need[PR_G], p->need[PR_Z], p->W[PR_G], p->W[PR_Z]);
        k_pw_marks_out<<<gb, TB, 0, st>>>(keep, n, p->marks + first);
        k_pr_emit<false><<<gb, TB, 0, st>>>(ops, n, cnt, keep, nullptr, state, nullptr, nullptr, 0u);
        CDCHK(hipGetLastError());
        const uint32_t rounds = h[S_ROUNDS];
        CDCHK(fetch(st, h, state));
        CDCHK(hipStreamSynchronize(st));
        for (int k = 0; k < PR_CLASSES; k++) cls[k] = h[S_CLS + k];
        h[S_ROUNDS] = rounds;
    }
    for (int k = 0; k < PR_CLASSES; k++) p->cls[k] += cls[k];
    p->rounds += h[S_ROUNDS];
    p->n_kept += kept;
    p->mark_feeds++;
    p->digest += feed.sum;
    p->pos = first;
    if (n_kept_here) *n_kept_here = (size_t)kept;
    return RV_OK;
}

int feed_impl(WinPruner* p, const DevAlloc& CA, const rv_op* ops, size_t n, rv_op* d_out, size_t cap, size_t* n_out, uint32_t* d_old_index) {
    hipStream_t st = p->st;
    Scratch S(CA, st);
    const uint32_t gb = blocks(n, TB);
    uint32_t* state = S.get<uint32_t>(S_WORDS);
    uint32_t *keep = S.get<uint32_t>(n), *at = S.get<uint32_t>(n);
    CDNEED(state && keep && at);
    std::vector<uint32_t> h(S_WORDS);
    uint64_t digest = 0;
    CDCHK(hipMemsetAsync(state, 0, S_WORDS * 4, st));
    CDCHK(hipMemsetAsync(state, 0xFF, 8, st));
    CDCHK(stage_digest(*p, ops, n, p->pos));
    k_pw_marks_in<<<gb, TB, 0, st>>>(p->marks + p->pos, n, keep);
    CDCHK((scan_excl<uint32_t, SumU32>(S, st, keep, at, n, &state[S_Q_TAIL])));  // (the word the kept count comes back in)
    CDCHK(fetch(st, h, state));
    CDCHK(stage_fetch_digest(*p, &digest));
    CDCHK(hipStreamSynchronize(st));
    const size_t kept = h[S_Q_TAIL];
    if (cap < kept) return RV_E_ARG;  // (nothing written, nothing moved)
    // (the class counts of this launch are not asked for: the keep words stand in for the reader counts)
    k_pr_emit<true><<<gb, TB, 0, st>>>(ops, n, keep, keep, at, state, reinterpret_cast<uint8_t*>(d_out), d_old_index, (uint32_t)p->pos);
    CDCHK(hipGetLastError());
    CDCHK(hipStreamSynchronize(st));
    p->digest += digest;
    p->pos += n;
    if (n_out) *n_out = kept;
    return RV_OK;
}
#undef CDCHK
#undef CDNEED

}  // namespace

int winprune_begin(hipStream_t st, const DevAlloc& A, uint64_t z64_wires, uint64_t gf2_wires, const uint32_t* const outs[2], const size_t n_outs[2],
                   WinPruner** out) {
    if (!stage_wires_ok(z64_wires, gf2_wires)) return RV_E_UNSUPPORTED;
    WinPruner* p = new WinPruner;
    p->W[PR_G] = gf2_wires, p->W[PR_Z] = z64_wires;
    for (int d = 0; d < 2; d++) p->outs[d].assign(outs[d], outs[d] + n_outs[d]);
    if (const int rc = stage_open(*p, st, A)) {
        winprune_destroy(p);
        return rc;
    }
    *out = p;
    return RV_OK;
}

int winprune_admit(WinPruner* p, int pass, size_t n) {
    if (!p->at(pass == 0 ? Phase::SCAN : pass == 1 ? Phase::MARK : Phase::FEED)) return RV_E_ARG;
    if (pass == 0) return stage_admit_first(*p, n);
    if (pass == 1) return n > p->pos ? RV_E_ARG : RV_OK;
    return n > p->total - p->pos ? RV_E_ARG : RV_OK;
}

int winprune_scan(WinPruner* p, const rv_op* d_ops, size_t n, size_t upload_bytes) {
    if (int rc = winprune_admit(p, 0, n)) return rc;
    if (!n) return RV_OK;
    return stage_settled(*p, stage_counted(*p, upload_bytes, [&](const DevAlloc& CA) { return scan_impl(p, CA, d_ops, n); }));
}

int winprune_scan_end(WinPruner* p) {
    if (!p->at(Phase::SCAN)) return RV_E_ARG;
    return stage_settled(*p, stage_counted(*p, 0, [&](const DevAlloc& CA) { return scan_end_impl(p, CA); }));
}

int winprune_mark(WinPruner* p, const rv_op* d_ops, size_t n, size_t upload_bytes, size_t* n_kept_here) {
    if (int rc = winprune_admit(p, 1, n)) return rc;
    if (n_kept_here) *n_kept_here = 0;
    if (!n) return RV_OK;
    return stage_settled(*p, stage_counted(*p, upload_bytes, [&](const DevAlloc& CA) { return mark_impl(p, CA, d_ops, n, n_kept_here); }));
}

int winprune_mark_end(WinPruner* p, rv_prune_info* info) {
    if (!p->at(Phase::MARK) || p->pos != 0 || p->digest != p->digest0) return RV_E_ARG;
    if (info) {
        *info = rv_prune_info{};
        info->n_kept = p->n_kept, info->n_dropped = p->total - p->n_kept;
        uint64_t* c = &info->dropped_gf2_mul;  // (the nine class counters lie in prune.h's order)
        for (int k = 0; k < PR_CLASSES; k++) c[k] = p->cls[k];
        info->device_rounds = (uint32_t)std::min<uint64_t>(p->rounds, 0xFFFFFFFFull), info->on_device = p->host_feeds ? 0u : 1u;
    }
    p->phase = Phase::FEED;
    p->pos = 0, p->digest = 0;
    return RV_OK;
}

int winprune_feed(WinPruner* p, const rv_op* d_ops, size_t n, size_t upload_bytes, rv_op* d_out, size_t cap, size_t* n_out, uint32_t* d_old_index) {
    if (int rc = winprune_admit(p, 2, n)) return rc;
    if (n_out) *n_out = 0;
    if (n)
        if (int rc = stage_settled(*p, stage_counted(*p, upload_bytes, [&](const DevAlloc& CA) {
                return feed_impl(p, CA, d_ops, n, d_out, cap, n_out, d_old_index);
            })))
            return rc;
    if (p->pos == p->total && !stage_pass_done(*p)) return RV_E_ARG;  // (the pass was not the scanned list)
    return RV_OK;
}

int winprune_rewind(WinPruner* p) {
    if (!p->at(Phase::FEED) || p->pos != p->total) return RV_E_ARG;
    p->pos = 0, p->digest = 0;
    return RV_OK;
}

int winprune_info(const WinPruner* p, rv_pruner_info* info) {
    if (p->failed) return RV_E_ARG;
    *info = rv_pruner_info{};
    info->total_ops = p->phase == Phase::SCAN ? p->pos : p->total;
    info->n_kept = p->n_kept;
    info->state_bytes = p->state_bytes();
    info->peak_feed_bytes = p->peak_feed;
    info->mark_feeds = p->mark_feeds;
    info->host_feeds = p->host_feeds;
    return RV_OK;
}

void winprune_destroy(WinPruner* p) {
    if (!p) return;
    stage_close(*p);
    p->give(p->need[PR_G]), p->give(p->need[PR_Z]), p->give(p->marks);
    delete p;
}

}  // namespace rv
