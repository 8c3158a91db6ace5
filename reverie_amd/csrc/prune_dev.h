// Dead ops dropped on the GPU (prune_dev.hip): rv_ops_prune's records, old_index and info, byte for byte, for an op list in device
// memory.  The rule is in include/reverie_amd.h, the per-record decisions in prune.h, the steps in DESIGN §23 and at the head of
// prune_dev.hip.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "compile_dev.h"
#include "prune.h"

namespace rv {

// threads per workgroup of the peeling kernels
constexpr uint32_t PRUNE_WG = 256;
// the widest frontier the solo kernel (one workgroup) peels round after round inside one launch; a wider one takes a grid
constexpr uint32_t PRUNE_SOLO_LIMIT = 1024;
// peeling iterations (one solo and one wide launch each) between two looks of the host at the device words
constexpr uint32_t PRUNE_LOOK_INTERVAL = 4;
// workgroups of the wide round kernel (grid-stride over the frontier)
constexpr uint32_t PRUNE_WIDE_BLOCKS = 1024;
// layers after which the call gives up on the device, where RV_PRUNE_MAX_ROUNDS does not say otherwise: the device compiler's bound
constexpr uint32_t PRUNE_MAX_ROUNDS_DEFAULT = 65536;

// RV_PRUNE_MAX_ROUNDS, read now (a value that is no positive number below 2^32: the default)
uint32_t prune_max_rounds();
// out[0..4): emit launches, count-only passes, peeling launches, fall-backs of this process
void prune_launches(uint64_t out[4]);

// d_ops: n_ops records in device memory; outs: the two output lists (GF(2), Z64) in host memory; d_out (cap records) and d_old_index
// (cap entries) may be null (d_out null: count only).  Memory from A, given back before the call returns.  RV_OK (n_out and info
// filled when not null), the list's validation code, RV_E_ARG (an output index out of range, cap too small; d_out untouched),
// RV_E_UNSUPPORTED, RV_E_NOMEM or RV_E_DEVICE.  Runs on `st`; synchronises it before returning.
int prune_ops_device(hipStream_t st, const DevAlloc& A, const rv_op* d_ops, size_t n_ops, uint64_t z64_wires, uint64_t gf2_wires,
                     const uint32_t* const outs[2], const size_t n_outs[2], rv_op* d_out, size_t cap, size_t* n_out, uint32_t* d_old_index,
                     rv_prune_info* info);

}  // namespace rv
