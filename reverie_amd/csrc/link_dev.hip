// see link.h
//
// A program linked from circuit blocks by kernels.  The plan holds ONE array of records -- the blocks' lists end to end,
// then head, then tail -- and the tables below; every per-record decision is link.h's.
//   create   1. judge     one thread per block record: lk_judge against its block's stated counts (the block by binary search in the
//                         blocks' offsets), the smallest (position << 8 | code) by a 64-bit atomicMin, one per workgroup; the record's
//                         Input flag into ports[].
//            2. ports     scan_excl<SumU32> over ports[] (one entry more than records: the total), in place.  A block's records have
//                         consecutive entries, so a port's ordinal inside its block is its entry minus the block's first.
//            3. gather    one thread per instance: block_of checked (smallest (instance << 8 | code)), the block's record count,
//                         stated counts and port count into off[], Z[], G[], B[] (one entry more than instances, zero: the totals).
//            4. scans     scan_excl<SumU64> over each of the four, in place.  The host reads the codes and the totals, judges head
//                         and tail, and decides (5).
//            5. bind      one thread per binding: its instance (the last with B <= k: it has a port), its port's record (the last of
//                         the block whose port ordinal is <= the port: the Input itself), the domain, then the value against the
//                         result's wire count -- the smallest (k << 8 | code) -- or, for RV_LINK_WITNESS, the Input counts.
//   emit     one workgroup per tile of 256 output records.  Every thread computes the tile's first instance from values that are the
//            same across the workgroup (the last instance whose offset is <= the tile's first ordinal: such an instance is not empty,
//            because the next offset is larger), then finds its own instance by doubling steps from there -- one probe where blocks are
//            large, a handful where a tile spans hundreds of 1-record or empty instances.  It reads the block record, the port
//            ordinal and the binding, applies lk_rewrite, and lays the 24 bytes into the tile's LDS image at the position modulo 16
//            they have in d_ops; the image goes out in 16-byte stores, with an 8-byte piece at an end where d_ops is only 8-byte
//            aligned (lk_chunk).  Head and tail records are copied as they are.  The range's Input counts: a ballot per wavefront, one
//            LDS atomic per wavefront, one global atomic per workgroup and domain.
// All stores are plain vector stores.  Every instance re-reads its block: a block is a few MB and stays in L2 and the MALL.
#include "link.h"

#include <algorithm>
#include <new>
#include <vector>

namespace rv {
namespace {
#include "compile_dev_prims.inc"
[[maybe_unused]] const auto unused_sort = &radix_sort;  // (the scans are all this file takes from the building blocks)
static_assert(TB == (int)LINK_TILE && TILE == (int)LINK_SCAN_BLOCK, "the sizes rv_hook_link_tiles reports");

struct SumU64 {
    __device__ uint64_t operator()(uint64_t a, uint64_t b) const { return a + b; }
    static __device__ uint64_t id() { return 0; }
};

enum { W_ERR_BLOCK, W_ERR_INST, W_ERR_BIND, W_IN_GF2, W_IN_Z64, W_WORDS };

__device__ inline void load_op(const uint64_t* ops, uint64_t i, uint64_t w[3]) { w[0] = ops[i * 3], w[1] = ops[i * 3 + 1], w[2] = ops[i * 3 + 2]; }

__global__ __launch_bounds__(TB) void k_link_init(uint64_t* state, uint32_t words, uint64_t first_value, uint32_t firsts) {
    if (threadIdx.x < words) state[threadIdx.x] = threadIdx.x < firsts ? first_value : 0;
}

// the smallest of the workgroup's `err` into *slot (every thread calls it)
__device__ inline void min_to(uint64_t err, unsigned long long* s_err, uint64_t* slot) {
    if (threadIdx.x == 0) *s_err = LK_NO_ERR;
    __syncthreads();
    for (int s = 32; s > 0; s >>= 1) err = std::min(err, (uint64_t)__shfl_xor((unsigned long long)err, s));
    if ((threadIdx.x & 63u) == 0 && err != LK_NO_ERR) atomicMin(s_err, (unsigned long long)err);
    __syncthreads();
    if (threadIdx.x == 0 && *s_err != LK_NO_ERR) atomicMin((unsigned long long*)slot, *s_err);
}

// blk[0, n_blocks): off is nondecreasing from 0, so the block of record r is the last one whose off is <= r and that is not empty --
// the last with off <= r at all, because a later block starts above r
struct BlockOff {
    const LkBlock* blk;
    __device__ uint64_t operator[](uint64_t i) const { return blk[i].off; }
};

__global__ __launch_bounds__(TB) void k_link_judge(const uint64_t* ops, uint64_t n, const LkBlock* blk, uint64_t n_blocks, uint32_t* ports, uint64_t* state) {
    __shared__ unsigned long long s_err;
    const uint64_t r = (uint64_t)blockIdx.x * TB + threadIdx.x;
    uint64_t err = LK_NO_ERR;
    if (r < n) {
        const BlockOff offs{blk};
        const LkBlock& k = blk[lk_last_le(offs, 0, n_blocks, r)];
        uint64_t w[3];
        load_op(ops, r, w);
        const int code = lk_judge(w, k.z64_wires, k.gf2_wires);
        if (code) err = r << 8 | (uint64_t)code;
        ports[r] = lk_is_input(w[0]) ? 1u : 0u;  // (of a record with a code: nothing is made of it)
    } else if (r == n) {
        ports[r] = 0;
    }
    min_to(err, &s_err, &state[W_ERR_BLOCK]);
}

__global__ __launch_bounds__(TB) void k_link_gather(const uint32_t* block_of, uint64_t n_inst, const LkBlock* blk, uint64_t n_blocks, const uint32_t* ports,
                                                    uint64_t* off, uint64_t* Z, uint64_t* G, uint64_t* B, uint64_t* state) {
    __shared__ unsigned long long s_err;
    const uint64_t i = (uint64_t)blockIdx.x * TB + threadIdx.x;
    uint64_t err = LK_NO_ERR;
    if (i <= n_inst) {
        uint64_t v[4] = {0, 0, 0, 0};
        if (i < n_inst) {
            const uint32_t b = block_of[i];
            if (b < n_blocks) {
                const LkBlock k = blk[b];
                v[0] = k.n_ops, v[1] = k.z64_wires, v[2] = k.gf2_wires, v[3] = ports[k.off + k.n_ops] - ports[k.off];
            } else {
                err = i << 8 | (uint64_t)RV_E_ARG;
            }
        }
        off[i] = v[0], Z[i] = v[1], G[i] = v[2], B[i] = v[3];
    }
    min_to(err, &s_err, &state[W_ERR_INST]);
}

struct LkTables {
    const uint64_t* ops;     // the blocks' records, head, tail
    const LkBlock* blk;
    const uint32_t* ports;   // per block record (and one more): Input records before it in the array
    const uint32_t* block_of;
    const uint32_t* bindings;
    const uint64_t *off, *Z, *G, *B;  // per instance (and one more: the totals), exclusive
    uint64_t n_inst;
};

__global__ __launch_bounds__(TB) void k_link_bind(LkTables T, uint64_t n_bind, uint64_t z64_wires, uint64_t gf2_wires, uint64_t* state) {
    __shared__ unsigned long long s_err;
    __shared__ unsigned int s_in[2];
    if (threadIdx.x < 2) s_in[threadIdx.x] = 0;
    const uint64_t k = (uint64_t)blockIdx.x * TB + threadIdx.x;
    uint64_t err = LK_NO_ERR;
    bool wit[2] = {false, false};
    if (k < n_bind) {
        const uint64_t i = lk_last_le(T.B, 0, T.n_inst, k);
        const LkBlock b = T.blk[T.block_of[i]];
        const uint32_t* po = T.ports + b.off;
        const uint32_t port = (uint32_t)(k - T.B[i]) + po[0];
        const uint64_t r = lk_last_le(po, 0, b.n_ops, port);
        const bool gf2 = lk_dom(T.ops[(b.off + r) * 3]) == RV_DOM_GF2;
        const uint32_t v = T.bindings[k];
        if (v == RV_LINK_WITNESS) wit[gf2 ? 0 : 1] = true;
        else if ((uint64_t)v >= (gf2 ? gf2_wires : z64_wires)) err = k << 8 | (uint64_t)RV_E_WIRE_OOB;
    }
    min_to(err, &s_err, &state[W_ERR_BIND]);  // (its barriers stand between the zeroing of s_in and the atomics on it)
    for (int d = 0; d < 2; d++) {
        const unsigned long long m = __ballot(wit[d]);
        if ((threadIdx.x & 63u) == 0 && m) atomicAdd(&s_in[d], (unsigned int)__popcll(m));
    }
    __syncthreads();
    if (threadIdx.x < 2 && s_in[threadIdx.x]) atomicAdd((unsigned long long*)&state[W_IN_GF2 + threadIdx.x], (unsigned long long)s_in[threadIdx.x]);
}

struct LkEmit {
    uint64_t first, n;                      // the range
    uint64_t n_head, inst_ops;              // the list is head, inst_ops records of instances, tail
    uint64_t head_at, tail_at;              // where head and tail lie in T.ops (records)
    uint32_t zb, gb;                        // the bases
};

__global__ __launch_bounds__(TB) void k_link_emit(LkTables T, LkEmit E, uint64_t* counts, uint8_t* out) {
    __shared__ __attribute__((aligned(16))) uint8_t raw[LK_IMAGE];
    __shared__ unsigned int s_in[2];
    if (threadIdx.x < 2) s_in[threadIdx.x] = 0;
    const uint64_t t0 = (uint64_t)blockIdx.x * TB;  // the tile's first record, counted from E.first
    const uint32_t mine = (uint32_t)std::min<uint64_t>(TB, E.n - t0);
    uint8_t* g0 = out + t0 * 24;
    const uint32_t sh = (uint32_t)((uintptr_t)g0 & 15u);
    // the tile's first instance, where the tile reaches into the instances (the same value in every thread)
    const uint64_t j0 = E.first + t0, jn = j0 + mine;
    uint64_t i0 = 0;
    if (jn > E.n_head && j0 < E.n_head + E.inst_ops) i0 = lk_last_le(T.off, 0, T.n_inst, j0 > E.n_head ? j0 - E.n_head : 0);
    bool in[2] = {false, false};
    if (threadIdx.x < mine) {
        const uint64_t j = j0 + threadIdx.x;
        uint64_t w[3], o[3];
        if (j < E.n_head) {
            load_op(T.ops, E.head_at + j, o);
        } else if (j >= E.n_head + E.inst_ops) {
            load_op(T.ops, E.tail_at + (j - E.n_head - E.inst_ops), o);
        } else {
            const uint64_t k = j - E.n_head;
            const uint64_t i = lk_gallop(T.off, i0, T.n_inst, k);
            const LkBlock b = T.blk[T.block_of[i]];
            const uint64_t r = b.off + (k - T.off[i]);
            load_op(T.ops, r, w);
            uint32_t binding = 0;
            if (lk_is_input(w[0])) binding = T.bindings[T.B[i] + (T.ports[r] - T.ports[b.off])];
            lk_rewrite(w, E.zb + (uint32_t)T.Z[i], E.gb + (uint32_t)T.G[i], binding, o);
        }
        uint64_t* img = reinterpret_cast<uint64_t*>(raw + sh + threadIdx.x * 24);
        img[0] = o[0], img[1] = o[1], img[2] = o[2];
        if (lk_is_input(o[0])) in[lk_dom(o[0]) == RV_DOM_GF2 ? 0 : 1] = true;
    }
    __syncthreads();
    const uint32_t span = sh + mine * 24;
    uint8_t* base = g0 - sh;  // 16-byte aligned; only [sh, span) of it is this tile's to write
    for (uint32_t c = threadIdx.x * 16; c < span; c += TB * 16) {
        const uint32_t kind = lk_chunk(c, sh, span);
        if (kind == 3) *reinterpret_cast<uint4*>(base + c) = *reinterpret_cast<const uint4*>(raw + c);
        else if (kind == 1) *reinterpret_cast<uint2*>(base + c) = *reinterpret_cast<const uint2*>(raw + c);
        else if (kind == 2) *reinterpret_cast<uint2*>(base + c + 8) = *reinterpret_cast<const uint2*>(raw + c + 8);
    }
    for (int d = 0; d < 2; d++) {
        const unsigned long long m = __ballot(in[d]);
        if ((threadIdx.x & 63u) == 0 && m) atomicAdd(&s_in[d], (unsigned int)__popcll(m));
    }
    __syncthreads();
    if (threadIdx.x < 2 && s_in[threadIdx.x]) atomicAdd((unsigned long long*)&counts[threadIdx.x], (unsigned long long)s_in[threadIdx.x]);
}

}  // namespace

struct LinkPlan {
    hipStream_t st;
    DevAlloc A;
    std::vector<void*> held;  // the plan's device arrays
    LkTables T = {};
    LkEmit E = {};
    uint64_t* counts = nullptr;  // the two Input counts of an emit
    rv_link_info info = {};
};

const rv_link_info& link_plan_info(const LinkPlan* p) { return p->info; }

void link_plan_destroy(LinkPlan* p) {
    if (!p) return;
    (void)hipStreamSynchronize(p->st);
    for (void* q : p->held) p->A.release(p->A.self, q);
    delete p;
}

int link_plan_create(hipStream_t st, const DevAlloc& A, const rv_link_desc* d, uint64_t block_ops, uint32_t flags, int* code, LinkPlan** plan,
                     rv_link_info* info) {
    *plan = nullptr, *code = RV_OK;
    Scratch S(A, st);  // everything the plan will hold, released here unless the plan is made (keep_all)
    const uint64_t n_inst = d->n_instances, n_bind = d->n_bindings, n_rec = block_ops + d->n_head + d->n_tail;
    uint64_t* ops = S.get<uint64_t>(n_rec * 3);
    LkBlock* blk = S.get<LkBlock>(d->n_blocks);
    uint32_t* ports = S.get<uint32_t>(block_ops + 1);
    uint32_t* block_of = S.get<uint32_t>(n_inst);
    uint32_t* bindings = S.get<uint32_t>(n_bind);
    uint64_t* pre = S.get<uint64_t>(4 * (n_inst + 1));
    uint64_t* state = S.get<uint64_t>(W_WORDS);
    CDNEED(ops && blk && ports && block_of && bindings && pre && state);
    uint64_t *off = pre, *Z = pre + (n_inst + 1), *G = Z + (n_inst + 1), *B = G + (n_inst + 1);

    // the copies: the blocks' lists end to end, head, tail; the block table; the two instance tables
    std::vector<LkBlock> hb(d->n_blocks);
    const hipMemcpyKind ops_from = (flags & RV_LINK_BLOCKS_ON_DEVICE) ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice;
    const hipMemcpyKind tab_from = (flags & RV_LINK_TABLES_ON_DEVICE) ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice;
    uint64_t at = 0;
    for (uint64_t b = 0; b < d->n_blocks; b++) {
        const rv_link_block& k = d->blocks[b];
        hb[b] = LkBlock{at, k.n_ops, k.z64_wires, k.gf2_wires};
        if (k.n_ops) CDCHK(hipMemcpyAsync(ops + at * 3, k.ops, k.n_ops * sizeof(rv_op), ops_from, st));
        at += k.n_ops;
    }
    if (d->n_head) CDCHK(hipMemcpyAsync(ops + at * 3, d->head, d->n_head * sizeof(rv_op), hipMemcpyHostToDevice, st));
    if (d->n_tail) CDCHK(hipMemcpyAsync(ops + (at + d->n_head) * 3, d->tail, d->n_tail * sizeof(rv_op), hipMemcpyHostToDevice, st));
    if (d->n_blocks) CDCHK(hipMemcpyAsync(blk, hb.data(), d->n_blocks * sizeof(LkBlock), hipMemcpyHostToDevice, st));
    if (n_inst) CDCHK(hipMemcpyAsync(block_of, d->block_of, n_inst * sizeof(uint32_t), tab_from, st));
    if (n_bind) CDCHK(hipMemcpyAsync(bindings, d->bindings, n_bind * sizeof(uint32_t), tab_from, st));

    k_link_init<<<1, TB, 0, st>>>(state, W_WORDS, LK_NO_ERR, W_IN_GF2);
    k_link_judge<<<blocks(block_ops + 1, TB), TB, 0, st>>>(ops, block_ops, blk, d->n_blocks, ports, state);
    CDCHK(hipGetLastError());
    CDCHK((scan_excl<uint32_t, SumU32>(S, st, ports, ports, block_ops + 1, nullptr)));
    k_link_gather<<<blocks(n_inst + 1, TB), TB, 0, st>>>(block_of, n_inst, blk, d->n_blocks, ports, off, Z, G, B, state);
    CDCHK(hipGetLastError());
    for (uint64_t* a : {off, Z, G, B}) CDCHK((scan_excl<uint64_t, SumU64>(S, st, a, a, n_inst + 1, nullptr)));
    std::vector<uint64_t> h(W_WORDS), tot(4);
    CDCHK(fetch(st, h, state));
    for (int a = 0; a < 4; a++) CDCHK(hipMemcpyAsync(&tot[a], pre + a * (n_inst + 1) + n_inst, sizeof(uint64_t), hipMemcpyDeviceToHost, st));
    CDCHK(hipStreamSynchronize(st));

    // (2) the blocks' first code; (3), (4) head and tail; (5) the instances, the binding count, the wire counts
    if (h[W_ERR_BLOCK] != LK_NO_ERR) return *code = (int)(h[W_ERR_BLOCK] & 0xFFu), RV_OK;
    LkEnds ends;
    if ((*code = lk_judge_end(d->head, d->n_head, ends))) return RV_OK;
    if ((*code = lk_judge_end(d->tail, d->n_tail, ends))) return RV_OK;
    if (h[W_ERR_INST] != LK_NO_ERR) return *code = (int)(h[W_ERR_INST] & 0xFFu), RV_OK;
    if (n_bind != tot[3]) return *code = RV_E_ARG, RV_OK;
    rv_link_info res = {};
    if ((*code = lk_wire_counts(d, ends, tot[1], tot[2], &res.z64_wires, &res.gf2_wires))) return RV_OK;

    LkTables T = {ops, blk, ports, block_of, bindings, off, Z, G, B, n_inst};
    // (6) the bindings, and the Input counts of the ports left to the witness
    if (n_bind) {
        k_link_bind<<<blocks(n_bind, TB), TB, 0, st>>>(T, n_bind, res.z64_wires, res.gf2_wires, state);
        CDCHK(hipGetLastError());
        CDCHK(fetch(st, h, state));
        CDCHK(hipStreamSynchronize(st));
        if (h[W_ERR_BIND] != LK_NO_ERR) return *code = (int)(h[W_ERR_BIND] & 0xFFu), RV_OK;
    }
    res.n_ops = d->n_head + tot[0] + d->n_tail, res.n_instances = n_inst;
    res.n_input_gf2 = ends.in_gf2 + h[W_IN_GF2], res.n_input_z64 = ends.in_z64 + h[W_IN_Z64];

    LinkPlan* p = new (std::nothrow) LinkPlan{};
    CDNEED(p);
    p->st = st, p->A = A, p->T = T, p->info = res;
    p->E.n_head = d->n_head, p->E.inst_ops = tot[0], p->E.head_at = block_ops, p->E.tail_at = block_ops + d->n_head;
    p->E.zb = (uint32_t)d->z64_base, p->E.gb = (uint32_t)d->gf2_base;  // (they fit where there are instances: lk_wire_counts; unused elsewhere)
    p->counts = state;  // (two of its words, set anew by every emit)
    (void)hipStreamSynchronize(st);
    // (the scans' sums are work memory: they go back; the rest is the plan's)
    for (void* q : {(void*)ops, (void*)blk, (void*)ports, (void*)block_of, (void*)bindings, (void*)pre, (void*)state}) {
        p->held.push_back(q);
        S.ps.erase(std::find(S.ps.begin(), S.ps.end(), q));
    }
    *plan = p, *info = res;
    return RV_OK;
}

int link_plan_emit(LinkPlan* p, uint64_t first, uint64_t n, rv_op* d_ops, rv_link_piece* piece) {
    Scratch S(p->A, p->st, false);  // (CDCHK's word for "out of memory": nothing is taken here)
    LkEmit E = p->E;
    E.first = first, E.n = n;
    k_link_init<<<1, TB, 0, p->st>>>(p->counts, 2, 0, 0);
    if (n) k_link_emit<<<blocks(n, TB), TB, 0, p->st>>>(p->T, E, p->counts, reinterpret_cast<uint8_t*>(d_ops));
    CDCHK(hipGetLastError());
    std::vector<uint64_t> h(2);
    CDCHK(fetch(p->st, h, p->counts));
    CDCHK(hipStreamSynchronize(p->st));
    *piece = rv_link_piece{first, n, h[0], h[1]};
    return RV_OK;
}
#undef CDCHK
#undef CDNEED

}  // namespace rv
