// Constants folded in a list that passes through in windows (fold_win.hip): rv_ops_fold's records and counts, byte for byte, from one
// forward pass of feeds that carries one known byte and one value word per wire index and domain -- and, where the caller asks for
// it, a log of the rewritten records from which any window of the folded list can be made again, in any order.  The contract is
// rv_folder_*'s in include/reverie_amd.h, the window step is DESIGN §24.8 and fold.h.  Every call runs on the stream given at the
// beginning and leaves it idle.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "compile_dev.h"
#include "fold.h"

namespace rv {

struct WinFolder;

int winfold_begin(hipStream_t st, const DevAlloc& A, uint64_t z64_wires, uint64_t gf2_wires, bool keep_log, WinFolder** out);
// RV_E_NOMEM / RV_E_DEVICE from any call: the carried state may be half moved, only winfold_destroy is accepted afterwards.
// d_ops: n records in device memory; upload_bytes: what the caller holds for this feed beside them (counted into peak_feed_bytes);
// d_out: n records, null (count, and log, only) or d_ops
int winfold_feed(WinFolder* p, const rv_op* d_ops, size_t n, size_t upload_bytes, rv_op* d_out);
int winfold_end(WinFolder* p, rv_fold_info* info);
int winfold_rewind(WinFolder* p);
int winfold_replay(WinFolder* p, const rv_op* d_ops, size_t n, size_t upload_bytes, uint64_t first, rv_op* d_out);
int winfold_replay_end(WinFolder* p);
int winfold_info(const WinFolder* p, rv_folder_info* info);
// What a feed (pass 0) or a replay (pass 1) of n ops, the replay at ordinal `first`, would answer before it looks at the ops (RV_OK:
// it may come next; RV_E_ARG: out of order or beyond the list; RV_E_UNSUPPORTED: 2^31 ops, after which nothing more is accepted).
// The calls ask themselves; a caller asks before it uploads a host feed, and returns what it hears.
int winfold_admit(WinFolder* p, int pass, size_t n, uint64_t first);
void winfold_destroy(WinFolder* p);

}  // namespace rv
