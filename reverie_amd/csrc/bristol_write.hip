// see bristol_write.h
//
// Bristol text written by kernels, built like the program-file writer of bincode_dev.hip:
//   1. lengths   one thread per record: bw_judge's code and line length (0: an Input record, or a record with a code), the lengths
//                into lens[].  The same pass reduces, per workgroup in LDS and then with one atomic each: the sum of the lengths; the
//                smallest (position << 8 | code) of a record with a code (a 64-bit atomicMin: "first in list order" across
//                workgroups); and for a whole list the largest index named plus one (where the wire count is derived) and the end of the
//                leading Input run -- the smallest position of a record that is no Input and stands behind an Input or at the list's
//                head (a handful of candidates, so a handful of atomics).  Whether an Input lies in the run is read off its predecessor: an
//                Input behind a record that is no Input is behind the run, and the first Input behind the run is such a one, so the
//                smallest code found is the list's (later Inputs behind the run need not be told apart: nothing is written then).
//   2. scan      scan_excl<SumU32> over lens[], in place: where each line starts behind the header.
//   3. emit      a workgroup lays its 256 records' lines out in LDS (at most 256 x 41 bytes; block 0's image begins with the header
//                lines, at most 96 bytes) at the position modulo 16 their bytes have in d_text, and stores the image: 16-byte stores
//                for the aligned chunks that are wholly its own, bytes at its two ends, where a neighbour's line shares a chunk.
//                Every workgroup reads the state words itself: nothing is written for a list with a code, nor into a buffer
//                that is too small.
// Work memory: 4 bytes per record, the scan's sums, the state words.  All stores are plain vector stores.
#include "bristol_write.h"

#include <algorithm>
#include <vector>

namespace rv {
namespace {
#include "compile_dev_prims.inc"
[[maybe_unused]] const auto unused_sort = &radix_sort;  // (the scans are all this file takes from the building blocks)
static_assert(TB == (int)BRISTOL_WRITE_TILE && TILE == (int)BRISTOL_WRITE_SCAN_BLOCK, "the sizes rv_hook_bristol_write_tiles reports");

enum { W_ERR, W_TOTAL, W_NEED, W_RUN, W_WORDS };
constexpr uint32_t IMAGE = 16 + BW_MAX_HEADER + BRISTOL_WRITE_TILE * BW_MAX_LINE + 16;  // alignment, header, lines, the 16-byte readers' slack

__device__ inline void load_op(const uint64_t* ops, uint64_t i, uint64_t w[3]) { w[0] = ops[i * 3], w[1] = ops[i * 3 + 1], w[2] = ops[i * 3 + 2]; }
__device__ inline bool is_input(uint64_t w0) { return (w0 & 0xFFFFu) == 0; }  // GF(2), RV_OP_INPUT (reserved is bw_judge's to look at)
// a whole list: is the record before record i an Input (or is there none)?
__device__ inline bool behind_input(const uint64_t* ops, uint64_t i) { return i == 0 || is_input(ops[(i - 1) * 3]); }
// record i of this launch: is its position in the leading Input run?
__device__ inline bool in_run(const BwJob& J, const uint64_t* ops, uint64_t i, uint64_t w0) {
    if (!J.whole) return J.first_op + i < J.n_inputs;
    return is_input(w0) && behind_input(ops, i);
}
// what the header says, from the job or (a whole list) from the state words of the lengths pass
struct BwHead {
    uint64_t gates, wires, inputs;
};
__device__ inline BwHead head_of(const BwJob& J, const uint64_t* state) {
    BwHead h;
    h.inputs = J.whole ? state[W_RUN] : J.n_inputs;
    h.wires = J.n_wires ? J.n_wires : std::max(state[W_NEED], h.inputs);
    h.gates = J.total_ops - h.inputs;
    return h;
}

__global__ __launch_bounds__(TB) void k_bw_init(uint64_t* state, uint64_t n) {
    if (threadIdx.x < W_WORDS) state[threadIdx.x] = threadIdx.x == W_ERR ? BW_NO_ERR : threadIdx.x == W_RUN ? n : 0;
}

__global__ __launch_bounds__(TB) void k_bristol_lens(const uint64_t* ops, uint64_t n, BwJob J, uint32_t* lens, uint64_t* state) {
    __shared__ unsigned int s_sum;
    __shared__ unsigned long long s_err, s_need, s_run;
    if (threadIdx.x == 0) s_sum = 0, s_err = BW_NO_ERR, s_need = 0, s_run = ~0ull;
    __syncthreads();
    const uint64_t i = (uint64_t)blockIdx.x * TB + threadIdx.x;
    uint32_t l = 0;
    uint64_t need = 0, err = BW_NO_ERR, run = ~0ull;
    if (i < n) {
        uint64_t w[3];
        load_op(ops, i, w);
        const int code = bw_judge(w, J.first_op + i, in_run(J, ops, i, w[0]), J.n_wires, l, need);
        lens[i] = l;
        if (code) err = (J.first_op + i) << 8 | (uint64_t)code;
        if (J.whole && !is_input(w[0]) && behind_input(ops, i)) run = i;  // (the end of the run is such a record, and the first of them)
    }
    // a wavefront's share first (64 lanes), then one LDS atomic per wavefront and value
    for (int s = 32; s > 0; s >>= 1) {
        l += __shfl_xor(l, s);
        need = std::max(need, (uint64_t)__shfl_xor((unsigned long long)need, s));
        err = std::min(err, (uint64_t)__shfl_xor((unsigned long long)err, s));
        run = std::min(run, (uint64_t)__shfl_xor((unsigned long long)run, s));
    }
    if ((threadIdx.x & 63u) == 0) {
        atomicAdd(&s_sum, l);
        atomicMax(&s_need, (unsigned long long)need);
        atomicMin(&s_err, (unsigned long long)err);
        atomicMin(&s_run, (unsigned long long)run);
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        // (none of these waits for an answer; the largest index is wanted only where the wire count is derived)
        if (s_sum) atomicAdd((unsigned long long*)&state[W_TOTAL], (unsigned long long)s_sum);
        if (s_err != BW_NO_ERR) atomicMin((unsigned long long*)&state[W_ERR], s_err);
        if (s_need && !J.n_wires) atomicMax((unsigned long long*)&state[W_NEED], s_need);
        if (s_run != ~0ull) atomicMin((unsigned long long*)&state[W_RUN], s_run);
    }
}

__global__ __launch_bounds__(TB) void k_bristol_emit(const uint64_t* ops, uint64_t n, BwJob J, const uint32_t* offs, const uint64_t* state, uint64_t cap,
                                                     uint8_t* out) {
    __shared__ __attribute__((aligned(16))) uint8_t raw[IMAGE];
    __shared__ uint64_t s_end;
    if (state[W_ERR] != BW_NO_ERR) return;
    const BwHead h = head_of(J, state);
    if (bw_header_code(h.wires, h.inputs, J.n_outputs)) return;
    const uint32_t head = J.header ? bw_header_len(h.gates, h.wires, h.inputs, J.n_outputs) : 0;
    if (head + state[W_TOTAL] > cap) return;
    const uint64_t first = (uint64_t)blockIdx.x * TB, i = first + threadIdx.x;
    const uint32_t mine = (uint32_t)std::min<uint64_t>(TB, n > first ? n - first : 0);
    // the block's bytes: out[g0, g1); block 0's begin with the header lines
    const uint64_t g0 = blockIdx.x ? head + (uint64_t)offs[first] : 0;
    const uint32_t sh = (uint32_t)((uintptr_t)(out + g0) & 15u);
    if (threadIdx.x == 0 && mine == 0) s_end = head;  // (no record at all: the header alone)
    if (blockIdx.x == 0 && threadIdx.x == 0 && head) bw_header(h.gates, h.wires, h.inputs, J.n_outputs, [&](uint32_t k, uint8_t v) { raw[sh + k] = v; });
    if (threadIdx.x < mine) {
        uint64_t w[3], need;
        uint32_t l;
        load_op(ops, i, w);
        (void)bw_judge(w, J.first_op + i, in_run(J, ops, i, w[0]), J.n_wires, l, need);
        const uint64_t at = head + (uint64_t)offs[i];
        if (l) {
            uint8_t* dst = raw + sh + (uint32_t)(at - g0);
            bw_emit(w, [&](uint32_t k, uint8_t v) { dst[k] = v; });
        }
        if (threadIdx.x == mine - 1) s_end = at + l;
    }
    __syncthreads();
    const uint32_t span = sh + (uint32_t)(s_end - g0);
    uint8_t* base = out + g0 - sh;  // 16-byte aligned; only [sh, span) of it is this block's to write
    for (uint32_t c = threadIdx.x * 16; c < span; c += TB * 16) {
        if (c >= sh && c + 16 <= span) {
            *reinterpret_cast<uint4*>(base + c) = *reinterpret_cast<const uint4*>(raw + c);
        } else {
            for (uint32_t k = 0; k < 16; k++)
                if (c + k >= sh && c + k < span) base[c + k] = raw[c + k];
        }
    }
}

}  // namespace

int bristol_write_device(hipStream_t st, const DevAlloc& A, const rv_op* d_ops, size_t n_ops, const BwJob& job, uint8_t* d_text, uint64_t cap,
                         BristolWrite* res) {
    Scratch S(A, st);
    uint64_t* state = S.get<uint64_t>(W_WORDS);
    uint32_t* lens = S.get<uint32_t>(n_ops);
    CDNEED(state && lens);
    const uint64_t* ops = reinterpret_cast<const uint64_t*>(d_ops);
    const uint32_t grid = blocks(n_ops, TB);
    const uint64_t room = std::min<uint64_t>(cap, 0xFFFFFFFFull);

    k_bw_init<<<1, TB, 0, st>>>(state, n_ops);
    if (n_ops) {
        k_bristol_lens<<<grid, TB, 0, st>>>(ops, n_ops, job, lens, state);
        CDCHK(hipGetLastError());
        CDCHK((scan_excl<uint32_t, SumU32>(S, st, lens, lens, n_ops, nullptr)));  // (wraps only where nothing is written)
    }
    if (d_text) k_bristol_emit<<<grid, TB, 0, st>>>(ops, n_ops, job, lens, state, room, d_text);
    CDCHK(hipGetLastError());
    std::vector<uint64_t> h(W_WORDS);
    CDCHK(fetch(st, h, state));
    CDCHK(hipStreamSynchronize(st));
    *res = BristolWrite{};
    if (h[W_ERR] != BW_NO_ERR) {
        res->code = (int)(h[W_ERR] & 0xFFu), res->record = true, res->err_op = h[W_ERR] >> 8;
        return RV_OK;
    }
    const uint64_t inputs = job.whole ? h[W_RUN] : job.n_inputs;
    const uint64_t wires = job.n_wires ? job.n_wires : std::max(h[W_NEED], inputs);
    if ((res->code = bw_header_code(wires, inputs, job.n_outputs))) return RV_OK;
    res->bytes = (job.header ? bw_header_len(job.total_ops - inputs, wires, inputs, job.n_outputs) : 0) + h[W_TOTAL];
    res->written = d_text && res->bytes <= room;
    return RV_OK;
}
#undef CDCHK
#undef CDNEED

}  // namespace rv
