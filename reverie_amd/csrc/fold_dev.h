// Constants folded on the GPU (fold_dev.hip): rv_ops_fold's records and info, byte for byte, for an op list in device memory.  The
// rule is in include/reverie_amd.h, the per-record decisions in fold.h, the steps in DESIGN §24 and at the head of fold_dev.hip.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "compile_dev.h"
#include "fold.h"

namespace rv {

// threads per workgroup of the propagation kernels
constexpr uint32_t FOLD_WG = 256;
// the widest frontier the solo kernel (one workgroup) steps layer after layer inside one launch; a wider one takes a grid
constexpr uint32_t FOLD_SOLO_LIMIT = 1024;
// propagation iterations (one solo and one wide launch each) between two looks of the host at the device words
constexpr uint32_t FOLD_LOOK_INTERVAL = 4;
// workgroups of the wide round kernel (grid-stride over the frontier)
constexpr uint32_t FOLD_WIDE_BLOCKS = 1024;
// layers after which the call gives up on the device, where RV_FOLD_MAX_ROUNDS does not say otherwise
constexpr uint32_t FOLD_MAX_ROUNDS_DEFAULT = 65536;

// RV_FOLD_MAX_ROUNDS, read now (a value that is no positive number below 2^32: the default)
uint32_t fold_max_rounds();
// out[0..4): rewrite launches, count-only passes, propagation launches, fall-backs of this process
void fold_launches(uint64_t out[4]);
// the windowed call's launches count with them (which: the word of fold_launches)
void fold_count_launches(int which, uint64_t count);

// d_ops: n_ops records in device memory; d_out (n_ops records) may be null (count only) or d_ops (in place).  Memory from A, given
// back before the call returns.  RV_OK (info filled when not null), the list's validation code (d_out untouched), RV_E_UNSUPPORTED,
// RV_E_NOMEM or RV_E_DEVICE.  Runs on `st`; synchronises it before returning.
int fold_ops_device(hipStream_t st, const DevAlloc& A, const rv_op* d_ops, size_t n_ops, uint64_t z64_wires, uint64_t gf2_wires, rv_op* d_out,
                    rv_fold_info* info);

}  // namespace rv
