// Dead ops dropped from a list that passes through in windows (prune_win.hip): rv_ops_prune's records, old_index and class counts,
// byte for byte, from three passes of feeds -- a forward scan, the marks from the last window to the first, the kept records
// forwards.  The contract is rv_pruner_*'s in include/reverie_amd.h, the window step is DESIGN §23.8 and prune.h.  Every call runs
// on the stream given at the beginning and leaves it idle.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "compile_dev.h"
#include "prune.h"

namespace rv {

struct WinPruner;

// outs: the two output lists (GF(2), Z64) in host memory; they are copied
int winprune_begin(hipStream_t st, const DevAlloc& A, uint64_t z64_wires, uint64_t gf2_wires, const uint32_t* const outs[2], const size_t n_outs[2],
                   WinPruner** out);
// RV_E_NOMEM / RV_E_DEVICE from any call: the carried state may be half moved, only winprune_destroy is accepted afterwards.
// d_ops: n records in device memory; upload_bytes: what the caller holds for this feed beside them (counted into peak_feed_bytes)
int winprune_scan(WinPruner* p, const rv_op* d_ops, size_t n, size_t upload_bytes);
int winprune_scan_end(WinPruner* p);
int winprune_mark(WinPruner* p, const rv_op* d_ops, size_t n, size_t upload_bytes, size_t* n_kept_here);
int winprune_mark_end(WinPruner* p, rv_prune_info* info);
int winprune_feed(WinPruner* p, const rv_op* d_ops, size_t n, size_t upload_bytes, rv_op* d_out, size_t cap, size_t* n_out, uint32_t* d_old_index);
int winprune_rewind(WinPruner* p);
int winprune_info(const WinPruner* p, rv_pruner_info* info);
// What a feed of n ops to pass `pass` (0 scan, 1 mark, 2 emit) would answer before it looks at the ops (RV_OK: it may come next;
// RV_E_ARG: out of order or beyond the list; RV_E_UNSUPPORTED: 2^31 ops, after which nothing more is accepted).  The feeds ask
// themselves; a caller asks before it uploads a host feed, and returns what it hears.
int winprune_admit(WinPruner* p, int pass, size_t n);
void winprune_destroy(WinPruner* p);

}  // namespace rv
