// compile_dev.hip, part 1: what both domains' kernels and host phases are built from
constexpr int TB = 256;           // threads per workgroup of every kernel here
constexpr int SI = 8;             // items per thread of the scans and the radix sort
constexpr int TILE = TB * SI;     // items per workgroup
struct SumU32 {
    __device__ uint32_t operator()(uint32_t a, uint32_t b) const { return a + b; }
    static __device__ uint32_t id() { return 0; }
};
struct MaxU32 {
    __device__ uint32_t operator()(uint32_t a, uint32_t b) const { return a > b ? a : b; }
    static __device__ uint32_t id() { return 0; }
};

// ---- exclusive scan (reduce, scan of the workgroup sums, down-sweep) ----
template <class T, class Op>
__global__ __launch_bounds__(TB) void k_scan_up(const T* in, size_t n, T* sums) {
    Op op;
    __shared__ T sh[TB];
    const size_t base = (size_t)blockIdx.x * TILE + (size_t)threadIdx.x * SI;
    T acc = Op::id();
    for (int k = 0; k < SI; k++)
        if (base + k < n) acc = op(acc, in[base + k]);
    sh[threadIdx.x] = acc;
    __syncthreads();
    for (int s = TB / 2; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) sh[threadIdx.x] = op(sh[threadIdx.x], sh[threadIdx.x + s]);
        __syncthreads();
    }
    if (threadIdx.x == 0) sums[blockIdx.x] = sh[0];
}
template <class T, class Op>
__device__ T block_excl(T v, T* sh, T* total) {  // exclusive scan of one value per thread across the workgroup
    Op op;
    sh[threadIdx.x] = v;
    __syncthreads();
    for (int s = 1; s < TB; s <<= 1) {
        const T t = (int)threadIdx.x >= s ? sh[threadIdx.x - s] : Op::id();
        __syncthreads();
        sh[threadIdx.x] = op(sh[threadIdx.x], t);
        __syncthreads();
    }
    const T ex = threadIdx.x ? sh[threadIdx.x - 1] : Op::id();
    *total = sh[TB - 1];
    __syncthreads();
    return ex;
}
template <class T, class Op>
__global__ __launch_bounds__(TB) void k_scan_mid(T* sums, size_t nb, T* total) {
    Op op;
    __shared__ T sh[TB];
    T carry = Op::id();
    for (size_t c0 = 0; c0 < nb; c0 += TB) {
        const size_t i = c0 + threadIdx.x;
        T tot;
        const T ex = block_excl<T, Op>(i < nb ? sums[i] : Op::id(), sh, &tot);
        if (i < nb) sums[i] = op(carry, ex);
        carry = op(carry, tot);
    }
    if (threadIdx.x == 0 && total) *total = carry;
}
template <class T, class Op>
__global__ __launch_bounds__(TB) void k_scan_down(const T* in, T* out, size_t n, const T* sums) {
    Op op;
    __shared__ T sh[TB];
    const size_t base = (size_t)blockIdx.x * TILE + (size_t)threadIdx.x * SI;
    T v[SI];
    T acc = Op::id();
    for (int k = 0; k < SI; k++) {
        v[k] = base + k < n ? in[base + k] : Op::id();
        acc = op(acc, v[k]);
    }
    T tot;
    T run = op(sums[blockIdx.x], block_excl<T, Op>(acc, sh, &tot));
    for (int k = 0; k < SI; k++)
        if (base + k < n) {
            out[base + k] = run;
            run = op(run, v[k]);
        }
}

// ---- stable LSD radix sort of (key, value) pairs, 8 bits per pass ----
__global__ __launch_bounds__(TB) void k_rs_hist(const uint32_t* keys, size_t n, int shift, uint32_t* hist, uint32_t n_tiles) {
    __shared__ uint32_t h[256];
    h[threadIdx.x] = 0;
    __syncthreads();
    const size_t base = (size_t)blockIdx.x * TILE;
    for (int s = 0; s < SI; s++) {
        const size_t i = base + (size_t)s * TB + threadIdx.x;
        if (i < n) atomicAdd(&h[(keys[i] >> shift) & 255u], 1u);
    }
    __syncthreads();
    hist[(size_t)threadIdx.x * n_tiles + blockIdx.x] = h[threadIdx.x];
}
// items of a tile in order: sub-round s, then thread; the rank of an item among the equal digits before it comes from
// wavefront ballots (the lanes that share its digit) and the per-wavefront digit counts of the sub-round in LDS
__global__ __launch_bounds__(TB) void k_rs_scatter(const uint32_t* kin, const uint32_t* vin, uint32_t* kout, uint32_t* vout, size_t n, int shift,
                                                   const uint32_t* off, uint32_t n_tiles) {
    __shared__ uint32_t run[256];
    __shared__ uint32_t wc[TB / 64][256];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    run[threadIdx.x] = off[(size_t)threadIdx.x * n_tiles + blockIdx.x];
    const size_t base = (size_t)blockIdx.x * TILE;
    for (int s = 0; s < SI; s++) {
        for (int w = 0; w < TB / 64; w++) wc[w][threadIdx.x] = 0;
        __syncthreads();
        const size_t i = base + (size_t)s * TB + threadIdx.x;
        const bool valid = i < n;
        const uint32_t k = valid ? kin[i] : 0u;
        const uint32_t d = (k >> shift) & 255u;
        unsigned long long peers = __ballot(valid);
        for (int b = 0; b < 8; b++) {
            const unsigned long long bb = __ballot(valid && ((d >> b) & 1u));
            peers &= ((d >> b) & 1u) ? bb : ~bb;
        }
        const uint32_t rank = (uint32_t)__popcll(peers & ((1ull << lane) - 1ull));
        const uint32_t cnt = (uint32_t)__popcll(peers);
        if (valid && rank + 1 == cnt) wc[wave][d] = cnt;
        __syncthreads();
        if (valid) {
            uint32_t at = run[d] + rank;
            for (uint32_t w = 0; w < wave; w++) at += wc[w][d];
            kout[at] = k;
            vout[at] = vin[i];
        }
        __syncthreads();
        uint32_t add = 0;
        for (int w = 0; w < TB / 64; w++) add += wc[w][threadIdx.x];
        run[threadIdx.x] += add;
        __syncthreads();
    }
}

// step 1 of every pass over an op list that checks wire indices (compact_dev.hip, prune_dev_kernels.inc's pr_step1, compact_win.hip):
// the two fields of a SizeHint per op, for the max-scans that give the counts in force at every op.  (Not every file that takes
// the scans and the sort from here launches it.)
[[maybe_unused]] __global__ __launch_bounds__(TB) void k_pr_hints(const rv_op* ops, size_t n, uint32_t* hz, uint32_t* hg) {
    const size_t i = (size_t)blockIdx.x * TB + threadIdx.x;
    if (i >= n) return;
    const bool h = ops[i].domain == RV_DOM_SIZEHINT;
    hz[i] = h ? ops[i].a : 0u;
    hg[i] = h ? ops[i].b : 0u;
}

inline uint32_t blocks(size_t n, size_t per) { return (uint32_t)std::max<size_t>(1, (n + per - 1) / per); }
inline int bit_len(uint64_t v) {
    int b = 0;
    while (v) b++, v >>= 1;
    return b;
}

// device allocations of one compile, given back (after a stream sync) when it ends.  Per op, beside the caller's 24-byte op and the
// 48-byte gate records that stay with the circuit: counters 16, two key / value pairs of the sorts 16, producers 8, read counts,
// pending operands, consumer offsets and cursors 16, consumers 8, value 8 (the lazy-sum form: 16), level, materialised flag, frontier
// and computed-row index 16, the sorts' histograms 0.5: 89 bytes (lazy sums: 97); 8 bytes per wire for the writer segments, and a chunk
// 20 more for its write-back flags and last writers; RV_COMPILE_KEEP_WIRES: 4 bytes per GF(2) wire for the last writers, and the two wire
// tables that stay with the circuit (16 bytes per GF(2) wire, 4 per Z64 wire)
// (sync = false: a Scratch that outlives another one of the same stream and is destroyed right after it -- the stream is idle then)
struct Scratch {
    const DevAlloc& A;
    hipStream_t st;
    std::vector<void*> ps;
    bool failed = false, sync;
    Scratch(const DevAlloc& a, hipStream_t s, bool sync_ = true) : A(a), st(s), sync(sync_) {}
    template <class T>
    T* get(size_t count) {
        void* p = nullptr;
        if (failed || A.alloc(A.self, std::max<size_t>(count, 1) * sizeof(T), &p) != RV_OK) {
            failed = true;
            return nullptr;
        }
        ps.push_back(p);
        return (T*)p;
    }
    void keep_all() { ps.clear(); }  // the arrays are the caller's from here on
    ~Scratch() {
        if (sync) (void)hipStreamSynchronize(st);
        for (void* p : ps) A.release(A.self, p);
    }
};

template <class T, class Op>
hipError_t scan_excl(Scratch& S, hipStream_t st, const T* in, T* out, size_t n, T* d_total) {
    const uint32_t nb = blocks(n, TILE);
    T* sums = S.get<T>(nb);
    if (!sums) return hipErrorOutOfMemory;
    k_scan_up<T, Op><<<nb, TB, 0, st>>>(in, n, sums);
    k_scan_mid<T, Op><<<1, TB, 0, st>>>(sums, nb, d_total);
    k_scan_down<T, Op><<<nb, TB, 0, st>>>(in, out, n, sums);
    return hipGetLastError();
}
// sorts (k[0], v[0]) by the low `bits` bits of the keys (stable); the result is left in (k[*which], v[*which])
hipError_t radix_sort(Scratch& S, hipStream_t st, uint32_t* k[2], uint32_t* v[2], size_t n, int bits, int* which) {
    const uint32_t nt = blocks(n, TILE);
    uint32_t* hist = S.get<uint32_t>((size_t)256 * nt);
    if (!hist) return hipErrorOutOfMemory;
    int cur = 0;
    for (int shift = 0; shift < std::max(bits, 1); shift += 8) {
        k_rs_hist<<<nt, TB, 0, st>>>(k[cur], n, shift, hist, nt);
        hipError_t e = scan_excl<uint32_t, SumU32>(S, st, hist, hist, (size_t)256 * nt, nullptr);
        if (e != hipSuccess) return e;
        k_rs_scatter<<<nt, TB, 0, st>>>(k[cur], v[cur], k[cur ^ 1], v[cur ^ 1], n, shift, hist, nt);
        cur ^= 1;
    }
    *which = cur;
    return hipGetLastError();
}

// ---- the host phases' error returns (S: the phase's work Scratch; #undef at the end of compile_dev.hip) ----
#define CDCHK(x)                                               \
    do {                                                       \
        if ((x) != hipSuccess) {                               \
            (void)hipGetLastError();                           \
            return S.failed ? RV_E_NOMEM : RV_E_DEVICE;        \
        }                                                      \
    } while (0)
#define CDNEED(p) \
    if (!(p)) return RV_E_NOMEM
// v (sized by the caller, and left alone until the stream is synchronised) = that many elements of device memory
template <class Vec>
hipError_t fetch(hipStream_t st, Vec& v, const void* src) {
    return v.empty() ? hipSuccess : hipMemcpyAsync(v.data(), src, v.size() * sizeof(typename Vec::value_type), hipMemcpyDeviceToHost, st);
}

// ---- the lap timer: HIP events on the compile's stream, made only when the caller wants DevCompileLaps ----
// The marks (fill_laps turns them into DevCompileLaps).  A GF(2)-only compile makes and records the first LAP_GF2_MARKS alone; in a mixed
// compile the split comes before LAP_BEGIN, the Z64 levels sit inside [LAP_DAG, LAP_LEVELS) and the Z64 tables follow LAP_DOWNLOADED.
enum { LAP_BEGIN, LAP_CLASSIFIED, LAP_DAG, LAP_LEVELS, LAP_TABLES, LAP_DOWNLOADED, LAP_GF2_MARKS, LAP_SPLIT = LAP_GF2_MARKS, LAP_SPLIT_END,
       LAP_Z64_LEVELS, LAP_Z64_LEVELS_END, LAP_Z64_TABLES, LAP_Z64_TABLES_END, LAP_MARKS };
struct LapTimer {
    hipStream_t st;
    bool wanted;
    int n = 0;  // events made
    hipEvent_t ev[LAP_MARKS] = {};
    LapTimer(hipStream_t s, bool w) : st(s), wanted(w) {}
    bool init(int marks) {  // the first `marks` events, once the request is in scope (false: one could not be made)
        for (; wanted && n < marks; n++)
            if (hipEventCreate(&ev[n]) != hipSuccess) return false;
        return true;
    }
    void mark(int k) {
        if (k < n) (void)hipEventRecord(ev[k], st);
    }
    float ms(int from, int to) const {  // (after a stream sync)
        float t = 0;
        if (to < n) (void)hipEventElapsedTime(&t, ev[from], ev[to]);
        return t;
    }
    ~LapTimer() {
        for (int k = 0; k < n; k++) (void)hipEventDestroy(ev[k]);
    }
};
