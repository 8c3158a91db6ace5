// Wire indices compacted by liveness on the GPU (compact_dev.hip): rv_ops_compact_wires' result, byte for byte, for an op list in
// device memory.  The rule is in include/reverie_amd.h, the parallel form in DESIGN §17 and at the head of compact_dev.hip.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "compile_dev.h"

namespace rv {

// ops one workgroup of the scans covers (the lengths the tests go around)
constexpr uint32_t COMPACT_TILE = 2048;

// d_ops, d_out: n_ops records in device memory (d_out may be d_ops); memory from A, given back before the call returns.  RV_OK (info
// filled when not null), the list's validation code (d_out untouched), RV_E_UNSUPPORTED, RV_E_NOMEM or RV_E_DEVICE.  Runs on `st`;
// synchronises it before returning.
int compact_ops_device(hipStream_t st, const DevAlloc& A, const rv_op* d_ops, size_t n_ops, uint64_t z64_wires, uint64_t gf2_wires, rv_op* d_out,
                       rv_compact_info* info);

}  // namespace rv
