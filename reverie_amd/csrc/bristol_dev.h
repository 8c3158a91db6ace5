// Bristol / Bristol Fashion gate lines parsed on the GPU (bristol_dev.hip): rv_bristol_parse's records, byte for byte, and its return
// code, for a text that lies in device memory.  The rule is in include/reverie_amd.h, the stages in DESIGN §18 and at the head of
// bristol_dev.hip.  The header lines are parsed on the host (bristol.cpp: one implementation for both parsers).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "compile_dev.h"

namespace rv {

// bytes of text one workgroup of the tile kernels covers, and gate lines one workgroup of the line kernels covers (the lengths the
// tests go around: rv_hook_bristol_tiles)
constexpr uint32_t BRISTOL_TILE_BYTES = 4096;
constexpr uint32_t BRISTOL_WG_LINES = 256;

struct BristolGates {
    int code = 0;          // RV_OK or the first bad gate line's code
    uint64_t gate_ops = 0;  // records the gate lines stand for (with RV_OK)
    uint64_t n_and = 0, n_xor = 0, n_inv = 0, n_other = 0;
    bool written = false;  // the records were written (the capacity sufficed)
};

// d_text[0, len): the whole text in device memory (len < 2^32), its gate lines from gates_offset on; n_gates, n_wires, n_inputs from the
// header.  d_ops / cap_ops: where the records go (null: nowhere); the assertion pairs of d_expected (device memory, n_pairs bytes, one
// per output wire; n_pairs 0: none) follow the gates.  Records are written only when there is no error and
// n_inputs + gate ops + 2 * pairs <= cap_ops -- decided on the device, so the stream is synchronised once, at the end.  Work memory
// from A, given back before the call returns.  RV_OK (res filled), RV_E_NOMEM or RV_E_DEVICE.
int bristol_gates_device(hipStream_t st, const DevAlloc& A, const uint8_t* d_text, size_t len, size_t gates_offset, uint64_t n_gates, uint64_t n_wires,
                         uint64_t n_inputs, const uint8_t* d_expected, uint64_t n_pairs, rv_op* d_ops, uint64_t cap_ops, BristolGates* res);

}  // namespace rv

// bristol.cpp: the header lines of text[0, len), a prefix of a text of full_len bytes that reaches the end of the first non-blank gate line
extern "C" int rv_internal_bristol_header(const char* text, size_t len, size_t full_len, int format, int has_expected, size_t n_expected,
                                          rv_bristol_info* info, size_t* gates_offset);
