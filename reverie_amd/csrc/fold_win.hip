// see fold_win.h
//
// fold_dev.hip's rule for a list that arrives in feeds.  Folding is a forward data-flow problem: one pass, and what a
// window hears from the ones before it is one known byte and one value word per wire index and domain (K, V).  The kernels of steps
// 1 - 6 are prune_dev_kernels.inc's and fold_dev_kernels.inc's, launched on the feed as they are launched on a whole list, with the
// tables as their Carried argument: a read with no producer in the feed is known exactly if its K byte is set.  Around them:
//
// Feed.  Step 1 with the counts in force carried from feed to feed as the classify kernel's seed, and the position-keyed digest of
// the feed (piece_sums.hip, as prune_win.hip sums it).  A SizeHint that raises a count grows the tables (k_fw_fill: known 0) before
// anything reads them.  Steps 2 - 5.  Then, in this order, because the rewrite may write over the records it read:
//   log      (RV_FOLDER_KEEP_LOG) one thread per op: a flag where the rewrite changes the record; the flags' exclusive sum; the host
//            reads the count and doubles the log if it must; one thread per op again: (ordinal, new record) to the log's end;
//   rewrite  step 6, or its count-only form;
//   tables   one thread per sorted pair of a domain's defining ops: the last pair of a key run stores its op's (known, value).
// A feed whose propagation reaches RV_FOLD_MAX_ROUNDS layers is copied down with the tables (the kernels have not touched them yet),
// stepped by fold.h's host sweep, and its records, tables and log entries uploaded.
//
// Replay (after end; any window, any order).  Two lower bounds in the log's ordinals, the source records copied to d_out unless in
// place, one thread per logged record of the slice: three 8-byte stores over the record it replaces.  No propagation, no tables.
#include "fold_win.h"

#include <stdlib.h>

#include <algorithm>
#include <utility>
#include <vector>

#include "fold_dev.h"
#include "prune_dev.h"
#include "win_stage.h"

namespace rv {
namespace {
#include "compile_dev_prims.inc"
static_assert(TB == (int)FOLD_WG && TB == (int)FOLD_TILE, "the kernels of fold_dev_kernels.inc are launched with TB threads");
static_assert(FOLD_SOLO_LIMIT % FOLD_WG == 0, "the solo kernel walks its frontier in whole strides");
#include "prune_dev_kernels.inc"

#include "fold_dev_kernels.inc"

enum { FW_LOG = FS_WORDS, FW_WORDS };      // the feed's words: the kernels', the changed records
constexpr size_t BOUNDS_AT = WIN_OWN_AT;   // the block's own quarter: a replay's slice of the log
constexpr size_t LOG_FIRST = 1024;         // the log's first capacity, in records

// ---- the tables ----
// entries [from, to) of one domain: nothing written yet, the zero wire
__global__ __launch_bounds__(TB) void k_fw_fill(uint8_t* K, uint64_t* V, uint64_t from, uint64_t to) {
    const uint64_t i = from + (uint64_t)blockIdx.x * TB + threadIdx.x;
    if (i < to) K[i] = 1, V[i] = 0ull;
}
// one thread per sorted pair of a domain's defining ops
__global__ __launch_bounds__(TB) void k_fw_tables(const uint32_t* sk, const uint32_t* sv, uint32_t nd, Fold f, uint8_t* K, uint64_t* V, uint64_t W) {
    const size_t j = (size_t)blockIdx.x * TB + threadIdx.x;
    if (j < nd) fd_table_update(sk, sv, nd, (uint32_t)j, f.known, f.val, K, V, W);
}

// ---- the log ----
__global__ __launch_bounds__(TB) void k_fw_changed(const rv_op* ops, size_t n, Fold f, Carried c, uint32_t* flag) {
    const size_t i = (size_t)blockIdx.x * TB + threadIdx.x;
    if (i >= n) return;
    const rv_op op = ops[i];
    bool kn[2] = {false, false};
    uint64_t v[2] = {0, 0};
    flag[i] = fd_changed(op, rewritten(op, i, f, c, kn, v)) ? 1u : 0u;
}
// (room: the entries the log has behind `ord`; a wrong count never becomes a store outside it)
__global__ __launch_bounds__(TB) void k_fw_log(const rv_op* ops, size_t n, Fold f, Carried c, const uint32_t* flag, const uint32_t* at, uint32_t first,
                                               uint32_t* ord, rv_op* rec, uint32_t room) {
    const size_t i = (size_t)blockIdx.x * TB + threadIdx.x;
    if (i >= n || flag[i] == 0u || at[i] >= room) return;
    const rv_op op = ops[i];
    bool kn[2] = {false, false};
    uint64_t v[2] = {0, 0};
    const rv_op now = rewritten(op, i, f, c, kn, v);
    const uint64_t* src = reinterpret_cast<const uint64_t*>(&now);
    uint64_t* dst = reinterpret_cast<uint64_t*>(rec + at[i]);
    ord[at[i]] = first + (uint32_t)i;
    dst[0] = src[0], dst[1] = src[1], dst[2] = src[2];
}

// ---- replay ----
// out[0], out[1]: the log's slice for the ordinals [first, first + n)
__global__ void k_fw_bounds(const uint32_t* ord, uint32_t n_log, uint64_t first, uint64_t n, uint32_t* out) {
    if (blockIdx.x == 0 && threadIdx.x < 2) out[threadIdx.x] = fd_log_lower_bound(ord, n_log, first + (threadIdx.x ? n : 0));
}
// one thread per logged record of the slice (ord, rec: at the slice's beginning); d_out is 8-byte aligned and so is every record of it
__global__ __launch_bounds__(TB) void k_fw_replay(const uint32_t* ord, const rv_op* rec, uint32_t count, uint64_t first, uint64_t n, rv_op* out) {
    const size_t j = (size_t)blockIdx.x * TB + threadIdx.x;
    if (j >= count) return;
    const uint64_t o = (uint64_t)ord[j] - first;
    if (ord[j] < first || o >= n) return;
    const uint64_t* src = reinterpret_cast<const uint64_t*>(rec + j);
    uint64_t* dst = reinterpret_cast<uint64_t*>(out + o);
    dst[0] = src[0], dst[1] = src[1], dst[2] = src[2];
}

}  // namespace

enum class Phase { FEED, ENDED };

struct WinFolder : WinStage {
    Phase phase = Phase::FEED;
    bool keep_log = false, first_pass = true;
    uint64_t W0[2] = {0, 0}, W[2] = {0, 0}, cap[2] = {0, 0};  // counts as declared, in force, the tables' entries ([PR_G], [PR_Z])
    uint8_t* K[2] = {nullptr, nullptr};
    uint64_t* V[2] = {nullptr, nullptr};
    uint32_t* log_ord = nullptr;
    rv_op* log_rec = nullptr;
    uint64_t log_n = 0, log_cap = 0;
    // this pass's sums
    uint64_t n_known = 0, cls[FD_CLASSES] = {}, rounds = 0, pass_host_feeds = 0;
    uint64_t feeds = 0, host_feeds = 0;
    // the replays since the last replay_end
    std::vector<std::pair<uint64_t, uint64_t>> replayed;
    uint64_t replay_digest = 0;

    bool at(Phase ph) const { return !failed && phase == ph; }
};

namespace {

// the tables hold at least `need` entries per domain afterwards; what they held stays, the new entries are known 0.  A table that
// has to grow at least doubles (up to the largest count a list may have in force), as the log does: a list whose SizeHints raise a
// count a little in many feeds copies its tables a logarithmic number of times.
int grow_tables(WinFolder* p, const uint64_t need[2]) {
    hipStream_t st = p->st;
    for (int d = 0; d < 2; d++) {
        if (need[d] <= p->cap[d] && p->K[d]) continue;
        const uint64_t want = std::max<uint64_t>(need[d], std::min<uint64_t>(2 * p->cap[d], 1ull << 31));
        uint8_t* k = (uint8_t*)p->take((size_t)want);
        uint64_t* v = (uint64_t*)p->take((size_t)want * 8);
        if (!k || !v) {
            p->give(k), p->give(v);
            return RV_E_NOMEM;
        }
        hipError_t e = hipSuccess;
        if (p->cap[d]) {
            e = hipMemcpyAsync(k, p->K[d], (size_t)p->cap[d], hipMemcpyDeviceToDevice, st);
            if (e == hipSuccess) e = hipMemcpyAsync(v, p->V[d], (size_t)p->cap[d] * 8, hipMemcpyDeviceToDevice, st);
        }
        if (e == hipSuccess && want > p->cap[d]) {
            k_fw_fill<<<blocks(want - p->cap[d], TB), TB, 0, st>>>(k, v, p->cap[d], want);
            e = hipGetLastError();
        }
        const hipError_t es = hipStreamSynchronize(st);  // (the old tables go while nothing reads them)
        p->give(p->K[d]), p->give(p->V[d]);
        p->K[d] = k, p->V[d] = v, p->cap[d] = want;
        if (e != hipSuccess || es != hipSuccess) {
            (void)hipGetLastError();
            return RV_E_DEVICE;
        }
    }
    return RV_OK;
}

// room for `more` entries behind the log's end: doubled, one sorted array before and after
int grow_log(WinFolder* p, uint64_t more) {
    if (p->log_n + more <= p->log_cap) return RV_OK;
    uint64_t cap = std::max<uint64_t>(p->log_cap, LOG_FIRST);
    while (cap < p->log_n + more) cap *= 2;
    uint32_t* o = (uint32_t*)p->take((size_t)cap * 4);
    rv_op* r = (rv_op*)p->take((size_t)cap * sizeof(rv_op));
    if (!o || !r) {
        p->give(o), p->give(r);
        return RV_E_NOMEM;
    }
    hipError_t e = hipSuccess;
    if (p->log_n) {
        e = hipMemcpyAsync(o, p->log_ord, (size_t)p->log_n * 4, hipMemcpyDeviceToDevice, p->st);
        if (e == hipSuccess) e = hipMemcpyAsync(r, p->log_rec, (size_t)p->log_n * sizeof(rv_op), hipMemcpyDeviceToDevice, p->st);
    }
    const hipError_t es = hipStreamSynchronize(p->st);
    p->give(p->log_ord), p->give(p->log_rec);
    p->log_ord = o, p->log_rec = r, p->log_cap = cap;
    if (e != hipSuccess || es != hipSuccess) {
        (void)hipGetLastError();
        return RV_E_DEVICE;
    }
    return RV_OK;
}

// the fall-back of one feed: the feed and the tables copied down, the host sweep, the records, the tables and the log entries uploaded
int feed_on_host(WinFolder* p, const rv_op* ops, size_t n, uint64_t first, rv_op* d_out, uint64_t cls[FD_CLASSES], uint64_t* n_known) {
    hipStream_t st = p->st;
    std::vector<rv_op> h(n), now(n);
    std::vector<uint8_t> hk[2] = {std::vector<uint8_t>((size_t)p->W[PR_G] + 1), std::vector<uint8_t>((size_t)p->W[PR_Z] + 1)};
    std::vector<uint64_t> hv[2] = {std::vector<uint64_t>((size_t)p->W[PR_G] + 1), std::vector<uint64_t>((size_t)p->W[PR_Z] + 1)};
    hipError_t e = hipMemcpyAsync(h.data(), ops, n * sizeof(rv_op), hipMemcpyDeviceToHost, st);
    for (int d = 0; d < 2; d++) {
        if (e == hipSuccess && p->W[d]) e = hipMemcpyAsync(hk[d].data(), p->K[d], (size_t)p->W[d], hipMemcpyDeviceToHost, st);
        if (e == hipSuccess && p->W[d]) e = hipMemcpyAsync(hv[d].data(), p->V[d], (size_t)p->W[d] * 8, hipMemcpyDeviceToHost, st);
    }
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e != hipSuccess) {
        (void)hipStreamSynchronize(st);
        (void)hipGetLastError();
        return RV_E_DEVICE;
    }
    uint8_t* const K[2] = {hk[PR_G].data(), hk[PR_Z].data()};
    uint64_t* const V[2] = {hv[PR_G].data(), hv[PR_Z].data()};
    fold_window_dense(h.data(), n, K, V, now.data(), cls, n_known);
    std::vector<uint32_t> lo;
    std::vector<rv_op> lr;
    if (p->keep_log)
        for (size_t i = 0; i < n; i++)
            if (fd_changed(h[i], now[i])) lo.push_back((uint32_t)(first + i)), lr.push_back(now[i]);
    if (!lo.empty())
        if (const int rc = grow_log(p, lo.size())) return rc;
    if (d_out) e = hipMemcpyAsync(d_out, now.data(), n * sizeof(rv_op), hipMemcpyHostToDevice, st);
    for (int d = 0; d < 2; d++) {
        if (e == hipSuccess && p->W[d]) e = hipMemcpyAsync(p->K[d], hk[d].data(), (size_t)p->W[d], hipMemcpyHostToDevice, st);
        if (e == hipSuccess && p->W[d]) e = hipMemcpyAsync(p->V[d], hv[d].data(), (size_t)p->W[d] * 8, hipMemcpyHostToDevice, st);
    }
    if (e == hipSuccess && !lo.empty()) {
        e = hipMemcpyAsync(p->log_ord + p->log_n, lo.data(), lo.size() * 4, hipMemcpyHostToDevice, st);
        if (e == hipSuccess) e = hipMemcpyAsync(p->log_rec + p->log_n, lr.data(), lr.size() * sizeof(rv_op), hipMemcpyHostToDevice, st);
    }
    const hipError_t es = hipStreamSynchronize(st);  // (also after an error: the vectors go while nothing reads them)
    if (e != hipSuccess || es != hipSuccess) {
        (void)hipGetLastError();
        return RV_E_DEVICE;
    }
    p->log_n += lo.size();
    fold_count_launches(3, 1);
    return RV_OK;
}

int feed_impl(WinFolder* p, const DevAlloc& CA, const rv_op* ops, size_t n, rv_op* d_out) {
    hipStream_t st = p->st;
    Scratch S(CA, st);
    const uint32_t gb = blocks(n, TB);
    const uint32_t max_rounds = fold_max_rounds();
    const uint64_t first = p->pos;
    uint32_t* state = S.get<uint32_t>(FW_WORDS);
    uint32_t *kbuf[2][2] = {}, *vbuf[2][2] = {};
    for (int k = 0; k < 2; k++) kbuf[0][k] = S.get<uint32_t>(n), vbuf[0][k] = S.get<uint32_t>(n);
    CDNEED(state && kbuf[0][0] && kbuf[0][1] && vbuf[0][0] && vbuf[0][1]);
    std::vector<uint32_t> h(FW_WORDS);

    // step 1, the counts in force carried in (the hints and their scans borrow the first sort's buffers)
    uint64_t W[2];
    WinFeed feed = {*p, first};
    if (const int rc = pr_step1(S, st, ops, n, state, FW_WORDS, p->W, kbuf[0], vbuf[0], &feed, h, W)) {
        p->failed = true;
        return rc;
    }
    if (const int rc = grow_tables(p, W)) return rc;
    p->W[PR_G] = W[PR_G], p->W[PR_Z] = W[PR_Z];
    const Carried c = {{p->K[PR_G], p->K[PR_Z]}, {p->V[PR_G], p->V[PR_Z]}};

    // step 2
    Writers w;
    if (const int rc = pr_step2(S, st, ops, n, W, h, kbuf, vbuf, &w)) return rc;

    // step 3
    Fold f = {S.get<uint32_t>(n), S.get<uint32_t>(n), S.get<uint32_t>(n), S.get<uint32_t>(n), S.get<uint64_t>(n)};
    uint32_t* queue = S.get<uint32_t>(n);
    CDNEED(f.pa && f.pb && f.pending && f.known && f.val && queue);
    k_fd_seed<<<gb, TB, 0, st>>>(ops, n, w, f, c, queue, state);
    k_pr_begin<<<1, 64, 0, st>>>(state);
    CDCHK(hipGetLastError());
    CDCHK(fetch(st, h, state));
    CDCHK(hipStreamSynchronize(st));

    uint64_t cls[FD_CLASSES] = {}, n_known = 0;
    uint32_t rounds = 0;
    bool on_host = false;
    if (!h[S_Q_TAIL] && !h[FS_UNWRITTEN]) {  // no op known at once and no known read from ahead of the feed: the records as they are
        if (d_out && d_out != ops) CDCHK(hipMemcpyAsync(d_out, ops, n * sizeof(rv_op), hipMemcpyDeviceToDevice, st));
    } else {
        if (h[S_Q_TAIL]) {
            // step 4
            const uint64_t n_pairs = (uint64_t)h[FS_PAIRS] | (uint64_t)h[FS_PAIRS + 1] << 32;
            on_host = n_pairs >= (1ull << 31);
            if (!on_host) {
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
                uint64_t launches = 0;
                const hipError_t pe = propagate(st, ops, n, w, f, c, rd, queue, state, max_rounds, h, &on_host, &launches);
                fold_count_launches(2, launches);
                CDCHK(pe);
                rounds = h[S_ROUNDS];
            }
        }
        if (on_host) {
            if (const int rc = feed_on_host(p, ops, n, first, d_out, cls, &n_known)) return rc;
        } else {
            // (every known op entered the queue once, and nothing else did)
            n_known = h[S_Q_TAIL];
            // the log, before the rewrite may write over the records (the queue and the pending counts have done their work: the
            // flags and their sums take their place)
            if (p->keep_log) {
                uint32_t *flag = queue, *at = f.pending;
                k_fw_changed<<<gb, TB, 0, st>>>(ops, n, f, c, flag);
                CDCHK((scan_excl<uint32_t, SumU32>(S, st, flag, at, n, &state[FW_LOG])));
                CDCHK(fetch(st, h, state));
                CDCHK(hipStreamSynchronize(st));
                const uint64_t more = h[FW_LOG];
                if (more) {
                    if (const int rc = grow_log(p, more)) return rc;
                    k_fw_log<<<gb, TB, 0, st>>>(ops, n, f, c, flag, at, (uint32_t)first, p->log_ord + p->log_n, p->log_rec + p->log_n, (uint32_t)more);
                    p->log_n += more;
                }
            }
            // step 6
            if (d_out) {
                k_fd_rewrite<true><<<gb, TB, 0, st>>>(ops, n, f, c, state, reinterpret_cast<uint8_t*>(d_out));
                fold_count_launches(0, 1);
            } else {
                k_fd_rewrite<false><<<gb, TB, 0, st>>>(ops, n, f, c, state, nullptr);
                fold_count_launches(1, 1);
            }
            CDCHK(hipGetLastError());
            CDCHK(fetch(st, h, state));
        }
    }
    if (!on_host) {
        // the tables, after everything that reads them
        for (int d = 0; d < 2; d++)
            if (w.nd[d]) k_fw_tables<<<blocks(w.nd[d], TB), TB, 0, st>>>(w.sk[d], w.sv[d], w.nd[d], f, p->K[d], p->V[d], W[d]);
        CDCHK(hipGetLastError());
        CDCHK(hipStreamSynchronize(st));
        if (h[S_Q_TAIL] || h[FS_UNWRITTEN])
            for (int k = 0; k < FD_CLASSES; k++) cls[k] = h[FS_CLS + k];
    } else {
        p->host_feeds++, p->pass_host_feeds++;
    }
    for (int k = 0; k < FD_CLASSES; k++) p->cls[k] += cls[k];
    p->n_known += n_known;
    p->rounds += rounds;
    p->feeds++;
    p->digest += feed.sum;
    p->pos += n;
    return RV_OK;
}

int replay_impl(WinFolder* p, const DevAlloc& CA, const rv_op* ops, size_t n, uint64_t first, rv_op* d_out) {
    hipStream_t st = p->st;
    Scratch S(CA, st);
    uint64_t digest = 0;
    uint32_t bounds[2] = {0, 0};
    uint32_t* d_bounds = (uint32_t*)(p->block + BOUNDS_AT);
    CDCHK(stage_digest(*p, ops, n, first));
    k_fw_bounds<<<1, 64, 0, st>>>(p->log_ord, (uint32_t)p->log_n, first, n, d_bounds);
    CDCHK(hipGetLastError());
    if (d_out != ops) CDCHK(hipMemcpyAsync(d_out, ops, n * sizeof(rv_op), hipMemcpyDeviceToDevice, st));
    CDCHK(stage_fetch_digest(*p, &digest));
    CDCHK(hipMemcpyAsync(bounds, d_bounds, 8, hipMemcpyDeviceToHost, st));
    CDCHK(hipStreamSynchronize(st));
    if (bounds[0] > bounds[1] || bounds[1] > p->log_n) return RV_E_DEVICE;
    const uint32_t count = bounds[1] - bounds[0];
    if (count) {
        k_fw_replay<<<blocks(count, TB), TB, 0, st>>>(p->log_ord + bounds[0], p->log_rec + bounds[0], count, first, n, d_out);
        CDCHK(hipGetLastError());
        CDCHK(hipStreamSynchronize(st));
    }
    p->replayed.emplace_back(first, (uint64_t)n);
    p->replay_digest += digest;
    return RV_OK;
}
#undef CDCHK
#undef CDNEED

// every entry of both tables: nothing written yet
int clear_tables(WinFolder* p) {
    for (int d = 0; d < 2; d++)
        if (p->cap[d]) k_fw_fill<<<blocks(p->cap[d], TB), TB, 0, p->st>>>(p->K[d], p->V[d], 0, p->cap[d]);
    if (hipGetLastError() != hipSuccess || hipStreamSynchronize(p->st) != hipSuccess) {
        (void)hipGetLastError();
        return RV_E_DEVICE;
    }
    return RV_OK;
}

void begin_pass(WinFolder* p) {
    p->W[PR_G] = p->W0[PR_G], p->W[PR_Z] = p->W0[PR_Z];
    p->pos = 0, p->digest = 0, p->log_n = 0;
    p->n_known = 0, p->rounds = 0, p->pass_host_feeds = 0;
    for (int k = 0; k < FD_CLASSES; k++) p->cls[k] = 0;
}

}  // namespace

int winfold_begin(hipStream_t st, const DevAlloc& A, uint64_t z64_wires, uint64_t gf2_wires, bool keep_log, WinFolder** out) {
    if (!stage_wires_ok(z64_wires, gf2_wires)) return RV_E_UNSUPPORTED;
    WinFolder* p = new WinFolder;
    p->keep_log = keep_log;
    p->W0[PR_G] = gf2_wires, p->W0[PR_Z] = z64_wires;
    begin_pass(p);
    int rc = stage_open(*p, st, A);
    if (rc == RV_OK) rc = grow_tables(p, p->W0);
    if (rc != RV_OK) {
        (void)hipGetLastError();
        winfold_destroy(p);
        return rc;
    }
    *out = p;
    return RV_OK;
}

int winfold_admit(WinFolder* p, int pass, size_t n, uint64_t first) {
    if (pass == 0) {
        if (!p->at(Phase::FEED)) return RV_E_ARG;
        if (!p->first_pass) return n > p->total - p->pos ? RV_E_ARG : RV_OK;
        return stage_admit_first(*p, n);
    }
    if (!p->at(Phase::ENDED) || !p->keep_log) return RV_E_ARG;
    return (first > p->total || n > p->total - first) ? RV_E_ARG : RV_OK;
}

int winfold_feed(WinFolder* p, const rv_op* d_ops, size_t n, size_t upload_bytes, rv_op* d_out) {
    if (int rc = winfold_admit(p, 0, n, 0)) return rc;
    if (n)
        if (int rc = stage_settled(*p, stage_counted(*p, upload_bytes, [&](const DevAlloc& CA) { return feed_impl(p, CA, d_ops, n, d_out); })))
            return rc;
    if (!p->first_pass && p->pos == p->total && !stage_pass_done(*p)) return RV_E_ARG;  // (the pass was not the first pass's list)
    return RV_OK;
}

int winfold_end(WinFolder* p, rv_fold_info* info) {
    if (!p->at(Phase::FEED)) return RV_E_ARG;
    if (!p->first_pass && !stage_pass_done(*p)) return RV_E_ARG;
    if (p->first_pass) p->total = p->pos, p->digest0 = p->digest, p->first_pass = false;
    if (info) {
        *info = rv_fold_info{};
        info->n_ops = p->total, info->n_known = p->n_known;
        uint64_t* c = &info->gf2_mul_to_const;  // (the nine class counters lie in fold.h's order)
        for (int k = 0; k < FD_CLASSES; k++) c[k] = p->cls[k];
        for (int k = 0; k < FD_REWRITTEN; k++) info->n_rewritten += c[k];
        info->device_rounds = (uint32_t)std::min<uint64_t>(p->rounds, 0xFFFFFFFFull), info->on_device = p->pass_host_feeds ? 0u : 1u;
    }
    p->phase = Phase::ENDED;
    p->replayed.clear(), p->replay_digest = 0;
    return RV_OK;
}

int winfold_rewind(WinFolder* p) {
    if (!p->at(Phase::ENDED)) return RV_E_ARG;
    if (const int rc = stage_settled(*p, clear_tables(p))) return rc;
    begin_pass(p);
    p->phase = Phase::FEED;
    return RV_OK;
}

int winfold_replay(WinFolder* p, const rv_op* d_ops, size_t n, size_t upload_bytes, uint64_t first, rv_op* d_out) {
    if (int rc = winfold_admit(p, 1, n, first)) return rc;
    if (!n) return RV_OK;
    return stage_settled(*p, stage_counted(*p, upload_bytes, [&](const DevAlloc& CA) { return replay_impl(p, CA, d_ops, n, first, d_out); }));
}

int winfold_replay_end(WinFolder* p) {
    if (!p->at(Phase::ENDED) || !p->keep_log) return RV_E_ARG;
    std::vector<std::pair<uint64_t, uint64_t>> r;
    r.swap(p->replayed);  // (the next round begins here, whatever this one was)
    const uint64_t digest = p->replay_digest;
    p->replay_digest = 0;
    std::sort(r.begin(), r.end());
    uint64_t at = 0;
    for (const auto& w : r) {
        if (w.first != at) return RV_E_ARG;
        at += w.second;
    }
    return (at == p->total && digest == p->digest0) ? RV_OK : RV_E_ARG;
}

int winfold_info(const WinFolder* p, rv_folder_info* info) {
    if (p->failed) return RV_E_ARG;
    *info = rv_folder_info{};
    info->total_ops = p->first_pass ? p->pos : p->total;
    info->state_bytes = WIN_BLOCK_BYTES + 9 * (p->cap[PR_G] + p->cap[PR_Z]);
    info->log_bytes = p->log_cap * (4 + sizeof(rv_op));
    info->log_records = p->log_n;
    info->peak_feed_bytes = p->peak_feed;
    info->feeds = p->feeds;
    info->host_feeds = p->host_feeds;
    return RV_OK;
}

void winfold_destroy(WinFolder* p) {
    if (!p) return;
    stage_close(*p);
    for (int d = 0; d < 2; d++) p->give(p->K[d]), p->give(p->V[d]);
    p->give(p->log_ord), p->give(p->log_rec);
    delete p;
}

}  // namespace rv
