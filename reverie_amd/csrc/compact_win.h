// Wire indices compacted by liveness for a list read in windows (compact_win.hip): compact_dev.hip's result, byte for byte, from
// two passes of feeds.  The contract is rv_compactor_*'s in include/reverie_amd.h, the carried state is DESIGN §17.5 and the head of
// compact_win.hip.  Every call runs on the stream given at the beginning and leaves it idle.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "compile_dev.h"

namespace rv {

struct WinCompactor;

int wincompact_begin(hipStream_t st, const DevAlloc& A, uint64_t z64_wires, uint64_t gf2_wires, WinCompactor** out);
// RV_E_NOMEM / RV_E_DEVICE from any call: the carried state may be half moved, only wincompact_destroy is accepted afterwards.
// d_ops: n records in device memory; upload_bytes: what the caller holds for this feed beside them (counted into peak_feed_bytes)
int wincompact_scan(WinCompactor* c, const rv_op* d_ops, size_t n, size_t upload_bytes);
int wincompact_scan_end(WinCompactor* c, int* again, rv_compact_info* info);
int wincompact_feed(WinCompactor* c, const rv_op* d_ops, size_t n, rv_op* d_out, size_t upload_bytes);
int wincompact_rewind(WinCompactor* c);
int wincompact_info(const WinCompactor* c, rv_compactor_info* info);  // RV_E_ARG once a scan feed refused the list
// What a scan / rewrite feed of n ops would answer before it looks at the ops (RV_OK: it may come next; RV_E_ARG: out of order or beyond
// the list; RV_E_UNSUPPORTED: 2^31 ops, after which a scan accepts nothing more).  The feeds ask themselves; a caller asks before it
// uploads a host feed, and returns what it hears.
int wincompact_admit_scan(WinCompactor* c, size_t n);
int wincompact_admit_feed(const WinCompactor* c, size_t n);
void wincompact_destroy(WinCompactor* c);

}  // namespace rv
