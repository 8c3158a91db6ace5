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
//                 they are needed), pending = the reads that have a producer.  A defining op that is known at once (fd_known of the reads without a producer: Const, a
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
// The kernels of steps 3 - 6 are fold_dev_kernels.inc's, shared with the windowed call (fold_win.hip); here they run without tables.
// The host reads device words after step 1, after step 3, inside the propagation loop and at the end.
#include "fold_dev.h"

#include <stdlib.h>

#include <algorithm>
#include <atomic>
#include <vector>

#include "prune_dev.h"
#include "win_stage.h"

namespace rv {
namespace {
#include "compile_dev_prims.inc"
static_assert(TB == (int)FOLD_WG && TB == (int)FOLD_TILE, "the sizes rv_hook_fold_limits reports");
static_assert(FOLD_SOLO_LIMIT % FOLD_WG == 0, "the solo kernel walks its frontier in whole strides");
#include "prune_dev_kernels.inc"

#include "fold_dev_kernels.inc"

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
    const uint64_t stated[2] = {gf2_wires, z64_wires};
    uint64_t W[2];
    if (const int rc = pr_step1(S, st, ops, n, state, FS_WORDS, stated, kbuf[0], vbuf[0], nullptr, h, W)) return rc;

    // step 2
    Writers w;
    if (const int rc = pr_step2(S, st, ops, n, W, h, kbuf, vbuf, &w)) return rc;

    // step 3
    Fold f = {S.get<uint32_t>(n), S.get<uint32_t>(n), S.get<uint32_t>(n), S.get<uint32_t>(n), S.get<uint64_t>(n)};
    uint32_t* queue = S.get<uint32_t>(n);
    CDNEED(f.pa && f.pb && f.pending && f.known && f.val && queue);
    const Carried none = {};  // (the whole list: a read without a producer is the zero wire)
    k_fd_seed<<<gb, TB, 0, st>>>(ops, n, w, f, none, queue, state);
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
        const hipError_t pe = propagate(st, ops, n, w, f, none, rd, queue, state, max_rounds, h, &gave_up, &launches);
        g_launches[2] += launches;
        CDCHK(pe);
        if (gave_up) return fold_on_host(S, st, ops, n, z64_wires, gf2_wires, d_out, info, h[S_ROUNDS]);
    }
    // (every known op entered the queue once, and nothing else did)
    const uint64_t n_known = h[S_Q_TAIL];
    const uint32_t rounds = h[S_ROUNDS];

    // step 6
    if (d_out) {
        k_fd_rewrite<true><<<gb, TB, 0, st>>>(ops, n, f, none, state, reinterpret_cast<uint8_t*>(d_out));
        g_launches[0]++;
    } else {
        k_fd_rewrite<false><<<gb, TB, 0, st>>>(ops, n, f, none, state, nullptr);
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

void fold_count_launches(int which, uint64_t count) { g_launches[which] += count; }

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
