// What the windowed stages of an op list share (compact_win.hip, prune_win.hip, fold_win.hip): a list passes through
// in feeds, several times, and the stage has to know that every pass was the same list.  Host code only.
//   block      WIN_BLOCK_BYTES of device memory that stay with the stage: a stage's own words at the start (the compactor's state),
//              the digest's cut pair, its sums, a quarter for the stage's own use (the folder's replay bounds).
//   digest     the position-keyed sum of a feed's records (piece_sums.hip), added up over a pass.  The first pass fixes the length
//              and the digest of the list (total, digest0); a later pass that ends with another digest was not that list.
//   admission  a feed is asked for before anything is uploaded or looked at: a call out of order is RV_E_ARG and moves nothing; a
//              first pass that reaches 2^31 ops is RV_E_UNSUPPORTED and closes the stage.
//   closing    a device or memory error in the middle of a call leaves the carried state half moved: `failed` is set, and only
//              the stage's destroy is accepted afterwards.
//   peak_feed  the most work memory one call held, the caller's uploaded copy of the feed included (peak_feed_bytes).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "compile_dev.h"
#include "dev_counting.h"
#include "piece_sums.h"

namespace rv {

constexpr size_t WIN_BLOCK_BYTES = 1024, WIN_CUT_AT = 256, WIN_SUMS_AT = 512, WIN_OWN_AT = 768;
constexpr uint64_t WIN_INDEX_LIMIT = 1ull << 31;  // an op's ordinal and a wire index fit 31 bits: op and wire counts stay below
static_assert(WIN_SUMS_AT + sizeof(PieceSums) <= WIN_OWN_AT, "the sums end before the stage's own quarter");

struct WinStage {
    hipStream_t st;
    DevAlloc A;
    uint8_t* block = nullptr;  // WIN_BLOCK_BYTES
    bool failed = false;
    uint64_t pos = 0, total = 0, digest = 0, digest0 = 0, cut_h[2] = {0, 0};
    size_t peak_feed = 0;

    // memory that stays with the stage (not counted into peak_feed)
    void* take(size_t bytes) {
        void* p = nullptr;
        return A.alloc(A.self, std::max<size_t>(bytes, 8), &p) == RV_OK ? p : nullptr;
    }
    void give(void* p) {
        if (p) A.release(A.self, p);
    }
};

inline bool stage_wires_ok(uint64_t z64_wires, uint64_t gf2_wires) { return z64_wires < WIN_INDEX_LIMIT && gf2_wires < WIN_INDEX_LIMIT; }

// the block allocated and cleared; after an error stage_close still has to be called
inline int stage_open(WinStage& s, hipStream_t st, const DevAlloc& A) {
    s.st = st, s.A = A;
    s.block = (uint8_t*)s.take(WIN_BLOCK_BYTES);
    if (!s.block) return RV_E_NOMEM;
    if (hipMemsetAsync(s.block, 0, WIN_BLOCK_BYTES, st) != hipSuccess || hipStreamSynchronize(st) != hipSuccess) return RV_E_DEVICE;
    return RV_OK;
}
// the stream idle, the block given back (what else the stage holds goes back after this)
inline void stage_close(WinStage& s) {
    (void)hipStreamSynchronize(s.st);
    s.give(s.block);
    s.block = nullptr;
}

// the digest sum of ops [0, n) of d_ops at the ordinals first .. goes to the block
inline hipError_t stage_digest(WinStage& s, const rv_op* d_ops, size_t n, uint64_t first) {
    s.cut_h[0] = 0, s.cut_h[1] = n;  // (the stage's own words: they outlive the copy)
    hipError_t e = hipMemcpyAsync(s.block + WIN_CUT_AT, s.cut_h, 16, hipMemcpyHostToDevice, s.st);
    if (e != hipSuccess) return e;
    launch_piece_sums(s.st, d_ops, (const uint64_t*)(s.block + WIN_CUT_AT), 1, n, first, (PieceSums*)(s.block + WIN_SUMS_AT));
    return hipGetLastError();
}
// *sum = that sum, once the stream is synchronised
inline hipError_t stage_fetch_digest(WinStage& s, uint64_t* sum) {
    return hipMemcpyAsync(sum, s.block + WIN_SUMS_AT, 8, hipMemcpyDeviceToHost, s.st);
}
// a feed on its way through step 1 of the prune/fold rule (prune_dev_kernels.inc's pr_step1): the stage whose digest it joins, its
// first op's ordinal, and the feed's sum when the step is done
struct WinFeed {
    WinStage& stage;
    uint64_t first;
    uint64_t sum = 0;
};

// fn(CA) with its work memory counted into peak_feed.  No exception leaves a call: host memory that cannot be had is RV_E_NOMEM,
// and stage_settled closes the stage as after any other one.
template <class Fn>
int stage_counted(WinStage& s, size_t upload_bytes, Fn&& fn) {
    size_t peak = 0;
    int rc;
    try {
        rc = counted_call(s.A, &peak, fn);
    } catch (...) {
        (void)hipStreamSynchronize(s.st);
        rc = RV_E_NOMEM;
    }
    s.peak_feed = std::max(s.peak_feed, peak + upload_bytes);
    return rc;
}

// a device or memory error closes the stage (closing(): what the stage drops then, on an idle stream)
template <class Hook>
int stage_settled(WinStage& s, int rc, Hook&& closing) {
    if (rc == RV_E_NOMEM || rc == RV_E_DEVICE) {
        (void)hipStreamSynchronize(s.st);
        closing();
        s.failed = true;
    }
    return rc;
}
inline int stage_settled(WinStage& s, int rc) {
    return stage_settled(s, rc, [] {});
}

// a feed of n ops to a first pass, whose length is not known yet
inline int stage_admit_first(WinStage& s, size_t n) {
    if (n >= WIN_INDEX_LIMIT || s.pos + n >= WIN_INDEX_LIMIT) {
        s.failed = true;
        return RV_E_UNSUPPORTED;
    }
    return RV_OK;
}

// the pass has reached the list's end and was the first pass's list
inline bool stage_pass_done(const WinStage& s) { return s.pos == s.total && s.digest == s.digest0; }

}  // namespace rv
