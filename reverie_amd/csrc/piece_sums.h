// What a streaming feed derives from the CONTENT of a piece, as sums over its ops (piece_sums.hip): the position-keyed digest
// (stream.inc: ops_digest), the ShareGen::next() calls (compile.h: count_masks) and the transcript events (count_events) -- and how
// many of its ops are not GF(2) (piece_all_gf2) or of no domain the device compiler takes under RV_COMPILE_DEVICE_Z64
// (compile.h: ops_without_b2a).  For a feed whose ops sit in device memory one kernel makes them for every piece in
// a single read of the ops; the host feeds keep their three loops.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "internal.h"

namespace rv {

struct PieceSums {
    uint64_t digest;            // ops_digest
    uint64_t masks2, masks64;   // count_masks
    uint64_t in2, rec2, pre2, on64, pre64;  // count_events
    uint64_t not_gf2;           // ops of another domain (0: piece_all_gf2)
    uint64_t not_z64;           // ops that are neither GF(2), Z64 nor SizeHint: B2A, unknown domains (0: piece_no_b2a; not asked under RV_COMPILE_DEVICE_B2A)
};
constexpr int PIECE_SUM_WORDS = 10;
static_assert(sizeof(PieceSums) == PIECE_SUM_WORDS * 8, "PieceSums is ten packed words");

// Piece i of n_pieces = ops [d_cut[i], d_cut[i + 1]) of d_ops (d_cut: n_pieces + 1 non-decreasing offsets in device memory); the op
// at offset j has stream position first_index + j.  Clears d_sums ([n_pieces] PieceSums) and adds every piece's sums into it, on `st`.
// max_piece: the longest piece (sizes the grid).
void launch_piece_sums(hipStream_t st, const rv_op* d_ops, const uint64_t* d_cut, size_t n_pieces, size_t max_piece, uint64_t first_index,
                       PieceSums* d_sums);

// The witness twin of the digest above (stream.inc: wit_digest), for the witnesses of a feed that sit in device memory: proof b of
// n_proofs (blockIdx.y) adds  sum_i mix(2 * (first2 + i), w2[b * stride2 + i] & 1) + sum_j mix(2 * (first64 + j) + 1, w64[b * stride64 + j])
// over i < n2 GF(2) bytes and j < n64 Z64 words into *acc[b] (one 64-bit atomic add per workgroup; the accumulators are not cleared).
// w2 is read byte by byte (alignment 1), w64 is 8-byte aligned; strides in elements.
struct WitSumsAcc {
    static constexpr uint32_t MAX = 64;
    uint64_t* acc[MAX];
};
void launch_wit_sums(hipStream_t st, const uint8_t* d_w2, uint64_t stride2, uint64_t n2, uint64_t first2, const uint64_t* d_w64, uint64_t stride64,
                     uint64_t n64, uint64_t first64, uint64_t* const* acc, size_t n_proofs);

}  // namespace rv
