// Part of api.hip (#included there, one translation unit): rv_prove_ops / rv_verify_ops and the context's content-addressed cache of compiled circuits.

// Proof::new / Proof::verify on the raw op list (proof/mod.rs:119-125,224-232): compile + prove / verify + release.
// The context keeps what these calls compile, and a kept circuit is found again BY CONTENT: every entry owns a copy of the op array
// it was compiled from and a hit is a full comparison against it (parallel memcmp on host threads, first difference ends it).
// Round 5 identified an op list by 128 bits of an unkeyed multiply-fold hash and never looked at the ops on a hit: two op lists
// with constructible equal hashes then shared one compiled circuit, and rv_verify_ops accepted a proof of one as a proof of the
// other where Proof::verify (proof/mod.rs:224-307) replays the caller's ops and rejects.  No hash is trusted any more, on either
// side: the prover must not silently prove another statement either.
static std::atomic<uint64_t> g_ops_cache_hits{0};
OpsCopy::OpsCopy(size_t n) : p((uint8_t*)malloc(n ? n : 1)), bytes(n) {
    if (!p) throw std::bad_alloc();
}
OpsCopy::~OpsCopy() { free(p); }
extern "C" uint64_t rv_hook_ops_cache_hits(void) { return g_ops_cache_hits.load(std::memory_order_relaxed); }
static unsigned ops_cmp_threads() {
    static const unsigned n_thr = [] {
        if (const char* e = getenv("RV_OPS_HASH_THREADS")) return (unsigned)std::max(atoi(e), 1);
        return std::min(16u, std::max(1u, std::thread::hardware_concurrency() / 2));
    }();
    return n_thr;
}
// fn(lo, hi) over [0, bytes) in 4 MiB pieces on up to ops_cmp_threads() host threads; a false return stops everybody
template <typename F>
static bool ops_for_pieces(size_t bytes, F fn) {
    constexpr size_t PIECE = (size_t)4 << 20;
    const size_t n_pieces = (bytes + PIECE - 1) / PIECE;
    const unsigned T = (unsigned)std::min<size_t>(ops_cmp_threads(), std::max<size_t>(n_pieces, 1));
    std::atomic<size_t> next{0};
    std::atomic<bool> go{true};
    auto work = [&] {
        for (size_t k; go.load(std::memory_order_relaxed) && (k = next.fetch_add(1, std::memory_order_relaxed)) < n_pieces;)
            if (!fn(k * PIECE, std::min(bytes, (k + 1) * PIECE))) go.store(false, std::memory_order_relaxed);
    };
    std::vector<std::thread> th;
    for (unsigned t = 1; t < T; t++) th.emplace_back(work);
    work();
    for (auto& t : th) t.join();
    return go.load();
}
static bool ops_same(const void* a, const void* b, size_t bytes) {
    if (a == b || bytes == 0) return true;
    return ops_for_pieces(bytes, [&](size_t lo, size_t hi) { return memcmp((const uint8_t*)a + lo, (const uint8_t*)b + lo, hi - lo) == 0; });
}
// host only (tests): what a cache lookup decides on -- 1 iff the two byte ranges are equal (threads and early exit as in a lookup)
extern "C" int rv_hook_ops_same(const void* a, const void* b, size_t bytes) {
    try {
        return (a && b) || !bytes ? (ops_same(a, b, bytes) ? 1 : 0) : -1;
    } catch (...) {
        return -1;
    }
}
// (what the compilers and circuit_upload make of an op list also depends on these; tests switch them between calls)
static std::string ops_knobs() {
    std::string knobs;
    for (const char* k : {"RV_LAZY_K", "RV_LAZY_SLACK", "RV_LAZY_BALANCE", "RV_NARROW", "RV_COMPILE_SEQ", "RV_LDS_RUN", "RV_LDS_QS"}) {
        const char* v = getenv(k);
        knobs += v ? v : "";
        knobs += ';';
    }
    return knobs;
}
static void ops_cache_evict_lru(rv_ctx* ctx) {
    size_t v = 0;
    for (size_t i = 1; i < ctx->ops_cache.size(); i++)
        if (ctx->ops_cache[i].stamp < ctx->ops_cache[v].stamp) v = i;
    rv_circuit_destroy(ctx->ops_cache[v].c);
    ctx->ops_cache.erase(ctx->ops_cache.begin() + (long)v);
}

// the compiled circuit of an op list, from the context's cache or compiled now (and kept: at most RV_OPS_CACHE entries, default 2,
// the least recently used one leaves BEFORE the new one is compiled, so that never more than RV_OPS_CACHE compiled circuits are
// resident; RV_OPS_CACHE=0: nothing is kept, *owned = the caller destroys it).  These calls mutate the context (header).
static int ops_cache_get(rv_ctx* ctx, const rv_op* ops, size_t n_ops, size_t z64_wires, size_t gf2_wires, uint32_t flags, rv_circuit** out, bool* hit,
                         bool* owned) {
    *hit = false;
    *owned = true;
    const size_t cap = getenv("RV_OPS_CACHE") ? (size_t)std::max(atoi(getenv("RV_OPS_CACHE")), 0) : 2;  // (read at every call: tests and bench switch it)
    if (!ctx || cap == 0 || !ops || n_ops < 1024) return rv_circuit_compile_ex(ctx, ops, n_ops, z64_wires, gf2_wires, flags, out);
    const size_t bytes = n_ops * sizeof(rv_op);
    const std::string knobs = ops_knobs();
    std::shared_ptr<OpsCopy> same;  // the kept copy of an entry with these very ops (the other compile form: shared, not copied)
    for (auto& e : ctx->ops_cache) {
        if (e.n_ops != n_ops || e.z64_wires != z64_wires || e.gf2_wires != gf2_wires) continue;
        if (e.ops != same && !ops_same(e.ops->p, ops, bytes)) continue;
        same = e.ops;
        if (e.flags != flags || e.knobs != knobs) continue;
        e.stamp = ++ctx->ops_clock;
        g_ops_cache_hits.fetch_add(1, std::memory_order_relaxed);
        *out = e.c;
        *hit = true;
        *owned = false;
        return RV_OK;
    }
    while (ctx->ops_cache.size() >= cap) ops_cache_evict_lru(ctx);
    // the copy is made BESIDE the compile (uninitialised memory, host threads of its own: the compile takes 60 - 70 ms, the copy 4)
    std::thread copier;
    if (!same) {
        same = std::make_shared<OpsCopy>(bytes);  // (bad_alloc: the callers answer RV_E_NOMEM)
        uint8_t* dst = same->p;
        copier = std::thread([=] {
            ops_for_pieces(bytes, [&](size_t lo, size_t hi) {
                memcpy(dst + lo, (const uint8_t*)ops + lo, hi - lo);
                return true;
            });
        });
    }
    struct Join {
        std::thread& t;
        ~Join() {
            if (t.joinable()) t.join();
        }
    } join_copier{copier};
    int rc = rv_circuit_compile_ex(ctx, ops, n_ops, z64_wires, gf2_wires, flags, out);
    if (rc == RV_E_NOMEM && !ctx->ops_cache.empty()) {  // room from the circuits kept for later, then once more
        while (!ctx->ops_cache.empty()) ops_cache_evict_lru(ctx);
        rc = rv_circuit_compile_ex(ctx, ops, n_ops, z64_wires, gf2_wires, flags, out);
    }
    if (copier.joinable()) copier.join();
    if (rc) return rc;
    ctx->ops_cache.push_back({same, knobs, n_ops, z64_wires, gf2_wires, flags, *out, ++ctx->ops_clock});
    *owned = false;
    return RV_OK;
}
extern "C" int rv_ctx_ops_cache_clear(rv_ctx* ctx) {
    if (!ctx) return RV_E_ARG;
    HIPCHK(hipSetDevice(ctx->device));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    for (auto& e : ctx->ops_cache) rv_circuit_destroy(e.c);
    ctx->ops_cache.clear();
    return RV_OK;
}

extern "C" int rv_prove_ops(rv_ctx* ctx, const rv_op* ops, size_t n_ops, const uint8_t* wit_gf2, size_t n_gf2, const uint64_t* wit_z64, size_t n_z64,
                            size_t z64_wires, size_t gf2_wires, const uint8_t* seeds, uint8_t** proof, size_t* proof_len) {
    if (!proof || !proof_len) return RV_E_ARG;
    rv_circuit* c = nullptr;
    bool hit = false, owned = true;
    // (under RV_COMPILE_DEVICE the prover's circuit is the device compiler's K = 1 form instead of the RV_COMPILE_WHOLE_PROVER
    // one: the proof bytes are the same, header.  The device compiler builds the lazy-sum form too; asking it for that here made
    // the cold call faster but not, measurably, the calls after it -- DESIGN.md 14.2)
    const uint32_t fl = (ctx && (ctx->compile_flags & RV_COMPILE_DEVICE)) ? (ctx->compile_flags & RV_COMPILE_DEVICE_BITS) : RV_COMPILE_WHOLE_PROVER;
    int rc = guarded([&] { return ops_cache_get(ctx, ops, n_ops, z64_wires, gf2_wires, fl, &c, &hit, &owned); });
    if (rc) return rc;
    // (the first proof of a circuit, or of one nobody keeps: without the early-corrections staging; a circuit seen before takes it)
    rc = guarded([&] { return rv_prove_impl(ctx, c, wit_host(wit_gf2, n_gf2, wit_z64, n_z64), seeds, proof, proof_len, nullptr, 0, /*allow_early=*/hit); });
    if (owned) rv_circuit_destroy(c);
    return rc;
}

extern "C" int rv_verify_ops(rv_ctx* ctx, const rv_op* ops, size_t n_ops, size_t z64_wires, size_t gf2_wires, const uint8_t* proof, size_t proof_len,
                             uint32_t flags, int* ok) {
    if (!ok) return RV_E_ARG;
    rv_circuit* c = nullptr;
    bool hit = false, owned = true;
    int rc;
    try {
        rc = ops_cache_get(ctx, ops, n_ops, z64_wires, gf2_wires, ctx ? (ctx->compile_flags & RV_COMPILE_DEVICE_BITS) : 0u, &c, &hit, &owned);
    } catch (...) {
        g_last_error = "out of host memory";
        return RV_E_NOMEM;
    }
    if (rc) return rc;
    rc = rv_verify_ex(ctx, c, proof, proof_len, flags, ok);
    if (owned) rv_circuit_destroy(c);
    return rc;
}
