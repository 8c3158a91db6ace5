// Multi-GPU proving inside the library -- part of api.hip's translation unit.
//
// The reference fans the 32 packed groups out over a rayon pool inside Proof::new (/root/reference/src/proof/mod.rs:
// 127-157) and meets again at exactly one point, combine_hashes over the 256 per-repetition digests (:160-172).  Here a
// communicator (one rank per GPU: one process per GPU, or one host thread per GPU) shards the repetitions, and that one
// meeting point is ONE ncclAllGather of 32-byte digests over RCCL/xGMI on the library's own stream; every rank then
// derives the challenge on its GPU (k_fs_challenge, shard form) and opens its own repetitions; the openings travel to
// rank 0 with ncclSend / ncclRecv straight into their place in the proof, which leaves rank 0's GPU in one copy.
//
// RCCL is bound at run time (dlopen): the library builds and loads on machines without it, and a process that
// already has an RCCL loaded (PyTorch ships one) keeps using that copy.
#include <dlfcn.h>

namespace {

typedef struct rv_nccl_comm* nccl_comm_t;
struct nccl_uid {
    char internal[128];
};
struct Rccl {
    void* so = nullptr;
    int (*GetUniqueId)(nccl_uid*) = nullptr;
    int (*CommInitRank)(nccl_comm_t*, int, nccl_uid, int) = nullptr;
    int (*CommInitAll)(nccl_comm_t*, int, const int*) = nullptr;
    int (*CommDestroy)(nccl_comm_t) = nullptr;
    int (*AllGather)(const void*, void*, size_t, int, nccl_comm_t, hipStream_t) = nullptr;
    int (*Send)(const void*, size_t, int, int, nccl_comm_t, hipStream_t) = nullptr;
    int (*Recv)(void*, size_t, int, int, nccl_comm_t, hipStream_t) = nullptr;
    int (*GroupStart)() = nullptr;
    int (*GroupEnd)() = nullptr;
    const char* (*GetErrorString)(int) = nullptr;
    std::string error;
};
constexpr int NCCL_UINT8 = 1;  // ncclUint8 (rccl.h)

static Rccl* rccl() {
    static Rccl R;
    static std::once_flag once;
    std::call_once(once, [] {
        std::vector<std::string> names;
        // RV_RCCL_PATH names THE library to bind (an explicit choice wins over a copy that happens to be in the process)
        if (const char* e = getenv("RV_RCCL_PATH")) {
            R.so = dlopen(e, RTLD_NOW | RTLD_GLOBAL);
            if (!R.so) {
                const char* m = dlerror();
                R.error = std::string("RV_RCCL_PATH could not be loaded: ") + (m ? m : "?");
                return;
            }
        }
        for (const char* n : {"librccl.so.1", "librccl.so"}) names.push_back(n);
        names.push_back("/opt/rocm/lib/librccl.so.1");
        // a copy that is already in the process (PyTorch's) first: one RCCL per process
        for (const std::string& n : names)
            if (!R.so) R.so = dlopen(n.c_str(), RTLD_NOW | RTLD_NOLOAD | RTLD_GLOBAL);
        for (const std::string& n : names)
            if (!R.so) R.so = dlopen(n.c_str(), RTLD_NOW | RTLD_GLOBAL);
        if (!R.so) {
            const char* e = dlerror();
            R.error = std::string("librccl could not be loaded: ") + (e ? e : "?");
            return;
        }
        auto sym = [&](const char* name) -> void* {
            void* p = dlsym(R.so, name);
            if (!p && R.error.empty()) R.error = std::string("librccl lacks ") + name;
            return p;
        };
        R.GetUniqueId = (decltype(R.GetUniqueId))sym("ncclGetUniqueId");
        R.CommInitRank = (decltype(R.CommInitRank))sym("ncclCommInitRank");
        R.CommInitAll = (decltype(R.CommInitAll))sym("ncclCommInitAll");
        R.CommDestroy = (decltype(R.CommDestroy))sym("ncclCommDestroy");
        R.AllGather = (decltype(R.AllGather))sym("ncclAllGather");
        R.Send = (decltype(R.Send))sym("ncclSend");
        R.Recv = (decltype(R.Recv))sym("ncclRecv");
        R.GroupStart = (decltype(R.GroupStart))sym("ncclGroupStart");
        R.GroupEnd = (decltype(R.GroupEnd))sym("ncclGroupEnd");
        R.GetErrorString = (decltype(R.GetErrorString))sym("ncclGetErrorString");
    });
    return &R;
}

static int nccl_fail(int code, const char* what) {
    Rccl* R = rccl();
    g_last_error = std::string(what) + " failed: " + (R->GetErrorString ? R->GetErrorString(code) : "?");
    return RV_E_DEVICE;
}
#define NCCLCHK(x)                              \
    do {                                        \
        int r_ = (x);                           \
        if (r_ != 0) return nccl_fail(r_, #x);  \
    } while (0)

}  // namespace

struct rv_comm {
    rv_ctx* ctx = nullptr;
    nccl_comm_t comm = nullptr;
    int world = 1, rank = 0;
    uint8_t* d_allh = nullptr;  // [256][32] gathered digests
    // rv_verify_sharded: this rank's part (its groups' slot digests, then a VERIFY_TRAILER-byte trailer that carries its
    // zero-check flag) and every rank's, gathered in rank order
    uint8_t *d_vmine = nullptr, *d_vall = nullptr;
};
constexpr size_t VERIFY_TRAILER = 32;

extern "C" int rv_comm_unique_id(uint8_t id[RV_COMM_ID_BYTES]) {
    if (!id) return RV_E_ARG;
    Rccl* R = rccl();
    if (!R->error.empty()) {
        g_last_error = R->error;
        return RV_E_DEVICE;
    }
    nccl_uid u;
    NCCLCHK(R->GetUniqueId(&u));
    memcpy(id, u.internal, RV_COMM_ID_BYTES);
    return RV_OK;
}

static int comm_wrap(rv_ctx* ctx, nccl_comm_t c, int world, int rank, rv_comm** out) {
    rv_comm* m = new rv_comm();
    m->ctx = ctx;
    m->comm = c;
    m->world = world;
    m->rank = rank;
    const size_t part = (size_t)RV_TOTAL_REPS / (size_t)world * 32 + VERIFY_TRAILER;
    int rc = dalloc(ctx, (size_t)RV_TOTAL_REPS * 32, &m->d_allh);
    if (!rc && (rc = dalloc(ctx, part, &m->d_vmine))) ctx->release(m->d_allh);
    if (!rc && (rc = dalloc(ctx, part * (size_t)world, &m->d_vall))) {
        ctx->release(m->d_allh);
        ctx->release(m->d_vmine);
    }
    if (rc) {
        delete m;
        return rc;
    }
    *out = m;
    return RV_OK;
}

extern "C" int rv_comm_create(rv_ctx* ctx, int world, int rank, const uint8_t id[RV_COMM_ID_BYTES], rv_comm** out) {
    if (!ctx || !out || !id || world < 1 || rank < 0 || rank >= world) return RV_E_ARG;
    *out = nullptr;
    if (RV_TOTAL_REPS % (8 * world)) return RV_E_ARG;  // whole packed groups per rank: 1, 2, 4, 8, 16 or 32 ranks
    Rccl* R = rccl();
    if (!R->error.empty()) {
        g_last_error = R->error;
        return RV_E_DEVICE;
    }
    HIPCHK(hipSetDevice(ctx->device));
    nccl_uid u;
    memcpy(u.internal, id, RV_COMM_ID_BYTES);
    nccl_comm_t c = nullptr;
    NCCLCHK(R->CommInitRank(&c, world, u, rank));
    return comm_wrap(ctx, c, world, rank, out);
}

extern "C" int rv_comm_create_all(rv_ctx* const* ctxs, int n, rv_comm** comms) {
    if (!ctxs || !comms || n < 1 || RV_TOTAL_REPS % (8 * n)) return RV_E_ARG;
    Rccl* R = rccl();
    if (!R->error.empty()) {
        g_last_error = R->error;
        return RV_E_DEVICE;
    }
    std::vector<int> devs((size_t)n);
    for (int i = 0; i < n; i++) {
        if (!ctxs[i]) return RV_E_ARG;
        devs[(size_t)i] = ctxs[i]->device;
        comms[i] = nullptr;
    }
    std::vector<nccl_comm_t> cs((size_t)n, nullptr);
    NCCLCHK(R->CommInitAll(cs.data(), n, devs.data()));
    for (int i = 0; i < n; i++) {
        int rc = comm_wrap(ctxs[i], cs[(size_t)i], n, i, &comms[i]);
        if (rc) return rc;
    }
    return RV_OK;
}

extern "C" void rv_comm_destroy(rv_comm* m) {
    if (!m) return;
    (void)hipSetDevice(m->ctx->device);
    (void)hipStreamSynchronize(m->ctx->stream);
    if (m->comm) (void)rccl()->CommDestroy(m->comm);
    m->ctx->release(m->d_allh);
    m->ctx->release(m->d_vmine);
    m->ctx->release(m->d_vall);
    delete m;
}

// shared_out (rv_prove_multi: all ranks are threads of ONE process): the framed proof's page-locked host buffer, `shared_cap` bytes.  Every
// rank then copies its own four sections straight to their places in it over its OWN PCIe link, beside the other ranks' copies: no
// ncclSend / ncclRecv, and rank 0 does not pay the whole proof's device-to-host copy behind its last kernel (proof/mod.rs:210-215 is
// the reference's gather point: `online` / `preprocessing` in ascending repetition order -- the offsets are a function of the challenge
// every rank has).  Rank 0 adds comm and the four length words.  Without it (rv_prove_sharded, one process per rank): the sections go
// to rank 0 by ncclSend / ncclRecv and leave in one copy.
static int prove_sharded_impl(rv_comm* m, const rv_circuit* c, const uint8_t* wit_gf2, size_t n_gf2, const uint64_t* wit_z64, size_t n_z64,
                              const uint8_t* seeds, uint8_t** proof, size_t* proof_len, uint8_t* shared_out = nullptr, size_t shared_cap = 0) {
    if (!m || !c || !seeds || !proof || !proof_len) return RV_E_ARG;
    *proof = nullptr;
    *proof_len = 0;
    rv_ctx* ctx = m->ctx;
    if (c->ctx != ctx) return RV_E_ARG;
    Rccl* R = rccl();
    HIPCHK(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    const uint32_t count = RV_TOTAL_REPS / (uint32_t)m->world, begin = (uint32_t)m->rank * count;
    rv_shard* s = nullptr;
    int rc = rv_shard_commit_impl(ctx, c, wit_host(wit_gf2, n_gf2, wit_z64, n_z64), seeds + (size_t)begin * 16, begin, count, &s, /*defer_sync=*/true);
    if (rc) return rc;  // (the other ranks are left waiting in the collective: the communicator is dead after a failed rank)
    uint8_t* d_mine = nullptr;   // this rank's openings (worst case: every one of min(40, count) repetitions opens)
    uint8_t* d_final = nullptr;  // rank 0: the framed proof
    uint8_t* out = nullptr;
    do {
        // ---- the one collective: 32-byte digests of every repetition to every rank, on the library's stream
        if (m->world > 1) {
            if (R->AllGather(s->d_h, m->d_allh, (size_t)count * 32, NCCL_UINT8, m->comm, st) != 0) {
                rc = nccl_fail(1, "ncclAllGather");
                break;
            }
        } else if (hipMemcpyAsync(m->d_allh, s->d_h, (size_t)RV_TOTAL_REPS * 32, hipMemcpyDeviceToDevice, st) != hipSuccess) {
            rc = RV_E_DEVICE;
            break;
        }
        size_t sz2 = 0, sz64 = 0;
        rv_circuit_record_sizes(c, &sz2, &sz64);
        const size_t cap = (size_t)std::min<uint32_t>(RV_ONLINE_REPS, count) * (sz2 + sz64) + (size_t)2 * count * 48;
        if ((rc = dalloc(ctx, std::max<size_t>(cap, 1), &d_mine))) break;
        // ---- challenge + this shard's openings on the device (one host synchronisation: comm, the map, the sizes)
        uint8_t comm_bytes[32], omit[RV_TOTAL_REPS];
        OpenArgs a;
        a.dst = d_mine;
        a.comm_out = comm_bytes;
        a.omit_out = omit;
        a.d_all_h = m->d_allh;
        OpenResult res;
        if ((rc = shard_open_impl(s, a, &res))) break;
        const size_t* const lens = res.lens;
        int err = 0;
        if (hipMemcpyAsync(&err, s->d_err, sizeof err, hipMemcpyDeviceToHost, st) != hipSuccess || hipStreamSynchronize(st) != hipSuccess) {
            rc = RV_E_DEVICE;
            break;
        }
        if (err) {
            rc = RV_E_WITNESS_INVALID;  // (every rank proves the same statement: they all see it)
            break;
        }
        // ---- every rank's section sizes follow from the challenge
        std::vector<std::array<size_t, 4>> all((size_t)m->world);
        for (int r = 0; r < m->world; r++) {
            size_t n_on = 0;
            for (uint32_t i = 0; i < count; i++) n_on += omit[(size_t)r * count + i] < 8;
            all[(size_t)r] = {n_on * sz2, (count - n_on) * 48, n_on * sz64, (count - n_on) * 48};
        }
        for (int k = 0; k < 4; k++)
            if (all[(size_t)m->rank][(size_t)k] != lens[k]) rc = RV_E_DEVICE;
        if (rc) break;
        if (shared_out) {
            size_t sec[4] = {0, 0, 0, 0}, mine[4] = {0, 0, 0, 0};  // section sizes of the whole proof; this rank's offsets inside them
            for (int r = 0; r < m->world; r++)
                for (int k = 0; k < 4; k++) {
                    if (r == m->rank) mine[k] = sec[k];
                    sec[k] += all[(size_t)r][(size_t)k];
                }
            size_t base[4], total = 32;
            for (int k = 0; k < 4; k++) {
                total += 8;
                base[k] = total;
                total += sec[k];
            }
            if (total > shared_cap) {
                rc = RV_E_DEVICE;
                break;
            }
            size_t off = 0;
            for (int k = 0; k < 4 && !rc; k++) {
                if (lens[k] && hipMemcpyAsync(shared_out + base[k] + mine[k], d_mine + off, lens[k], hipMemcpyDeviceToHost, st) != hipSuccess) rc = RV_E_DEVICE;
                off += lens[k];
            }
            if (!rc && hipStreamSynchronize(st) != hipSuccess) rc = hip_fail(hipGetLastError(), "sharded proof D2H (shared buffer)", __FILE__, __LINE__);
            if (rc) break;
            if (m->rank == 0) {
                memcpy(shared_out, comm_bytes, 32);
                frame_counts_at(shared_out, base);
                *proof = shared_out;
                *proof_len = total;
            }
            break;
        }
        if (m->rank != 0) {
            // the four sections of this rank, one send each (rank 0 posts the matching receives)
            if (R->GroupStart() != 0) {
                rc = nccl_fail(1, "ncclGroupStart");
                break;
            }
            size_t off = 0;
            for (int k = 0; k < 4; k++) {
                if (lens[k] && R->Send(d_mine + off, lens[k], NCCL_UINT8, 0, m->comm, st) != 0) rc = nccl_fail(1, "ncclSend");
                off += lens[k];
            }
            if (R->GroupEnd() != 0 && !rc) rc = nccl_fail(1, "ncclGroupEnd");
            if (!rc && hipStreamSynchronize(st) != hipSuccess) rc = RV_E_DEVICE;
            break;
        }
        // ---- rank 0: the framed proof, sections in place
        size_t sec[4] = {0, 0, 0, 0};
        for (int r = 0; r < m->world; r++)
            for (int k = 0; k < 4; k++) sec[k] += all[(size_t)r][(size_t)k];
        size_t base[4], total = 32;
        for (int k = 0; k < 4; k++) {
            total += 8;
            base[k] = total;
            total += sec[k];
        }
        if ((rc = dalloc(ctx, total, &d_final))) break;
        if (m->world > 1 && R->GroupStart() != 0) {
            rc = nccl_fail(1, "ncclGroupStart");
            break;
        }
        size_t at[4] = {base[0], base[1], base[2], base[3]};
        for (int r = 0; r < m->world; r++) {
            size_t off = 0;
            for (int k = 0; k < 4; k++) {
                const size_t n = all[(size_t)r][(size_t)k];
                if (n) {
                    if (r == 0) {
                        if (hipMemcpyAsync(d_final + at[k], d_mine + off, n, hipMemcpyDeviceToDevice, st) != hipSuccess) rc = RV_E_DEVICE;
                    } else if (R->Recv(d_final + at[k], n, NCCL_UINT8, r, m->comm, st) != 0) {
                        rc = nccl_fail(1, "ncclRecv");
                    }
                }
                at[k] += n;
                off += n;
            }
        }
        if (m->world > 1 && R->GroupEnd() != 0 && !rc) rc = nccl_fail(1, "ncclGroupEnd");
        if (rc) break;
        out = (uint8_t*)out_alloc(total);
        if (!out) {
            rc = RV_E_NOMEM;
            break;
        }
        if (hipMemcpyAsync(out, d_final, total, hipMemcpyDeviceToHost, st) != hipSuccess || hipStreamSynchronize(st) != hipSuccess) {
            rc = hip_fail(hipGetLastError(), "sharded proof D2H", __FILE__, __LINE__);
            break;
        }
        memcpy(out, comm_bytes, 32);
        frame_counts_at(out, base);
        *proof = out;
        *proof_len = total;
        out = nullptr;
    } while (0);
    ctx->collect();
    rv_free(out);
    ctx->release(d_mine);
    ctx->release(d_final);
    rv_shard_destroy(s);
    return rc;
}

extern "C" int rv_prove_sharded(rv_comm* m, const rv_circuit* c, const uint8_t* wit_gf2, size_t n_gf2, const uint64_t* wit_z64, size_t n_z64,
                                const uint8_t* seeds, uint8_t** proof, size_t* proof_len) {
    return guarded([&] { return prove_sharded_impl(m, c, wit_gf2, n_gf2, wit_z64, n_z64, seeds, proof, proof_len); });
}

// one process, n GPUs: a host thread per rank runs rv_prove_sharded; the proof is rank 0's
extern "C" int rv_prove_multi(rv_comm* const* comms, const rv_circuit* const* circuits, int n, const uint8_t* wit_gf2, size_t n_gf2,
                              const uint64_t* wit_z64, size_t n_z64, const uint8_t* seeds, uint8_t** proof, size_t* proof_len) {
    if (!comms || !circuits || n < 1 || !proof || !proof_len) return RV_E_ARG;
    uint8_t drawn[RV_TOTAL_REPS * RV_KEY_SIZE];
    if (!seeds) {  // every rank must use the same seeds: drawn once, here
        if (int rs = os_seeds(drawn, sizeof drawn)) return rs;
        seeds = drawn;
    }
    // the framed proof's size does not depend on the challenge (40 / 216): one page-locked buffer that every rank fills its part of
    if (!circuits[0]) return RV_E_ARG;
    const size_t total = whole_proof_layout(circuits[0]->cc).total;
    // RV_MULTI_SENDRECV=1: rv_prove_sharded's own gather instead (sections to rank 0 by ncclSend / ncclRecv, one copy out) -- what several
    // PROCESSES run; the multi-rank tests drive both forms through this call (read at every call)
    const bool sendrecv = getenv("RV_MULTI_SENDRECV") && atoi(getenv("RV_MULTI_SENDRECV")) != 0;
    uint8_t* shared = sendrecv ? nullptr : (uint8_t*)out_alloc(total);
    if (!sendrecv && !shared) return RV_E_NOMEM;
    std::vector<int> rcs((size_t)n, RV_OK);
    std::vector<uint8_t*> outs((size_t)n, nullptr);
    std::vector<size_t> lens((size_t)n, 0);
    std::vector<std::string> errs((size_t)n);
    auto run = [&](int i) {
        rcs[(size_t)i] = guarded([&] {
            return prove_sharded_impl(comms[i], circuits[i], wit_gf2, n_gf2, wit_z64, n_z64, seeds, &outs[(size_t)i], &lens[(size_t)i], shared, total);
        });
        if (rcs[(size_t)i]) errs[(size_t)i] = g_last_error;
    };
    std::vector<std::thread> th;
    for (int i = 1; i < n; i++) th.emplace_back(run, i);
    run(0);
    for (auto& t : th) t.join();
    int rc = RV_OK;
    for (int i = 0; i < n; i++)
        if (rcs[(size_t)i] && !rc) {
            rc = rcs[(size_t)i];
            g_last_error = errs[(size_t)i];
        }
    if (!rc && ((!sendrecv && outs[0] != shared) || lens[0] != total)) rc = RV_E_DEVICE;
    if (sendrecv)
        for (int i = 1; i < n; i++) rv_free(outs[(size_t)i]);
    if (rc) {
        rv_free(sendrecv ? outs[0] : shared);
        return rc;
    }
    *proof = outs[0];
    *proof_len = lens[0];
    return RV_OK;
}


// ---- multi-GPU verification: the verifier's 32 groups of eight slots dealt over the ranks, one all-gather of their digests

extern "C" int rv_verify_partition(int world, int rank, uint8_t groups[32], uint32_t* n_groups) {
    if (!groups || !n_groups || world < 1 || world > 32 || (32 % world) || rank < 0 || rank >= world) return RV_E_ARG;
    const int per = 32 / world, n_online = RV_ONLINE_REPS / 8;
    uint32_t n = 0;
    for (int g = rank; g < n_online; g += world) groups[n++] = (uint8_t)g;  // online groups round-robin, first
    // then the preprocessing groups in ascending order, each rank in turn filled up to `per`
    int next = n_online;
    for (int r = 0; r < rank; r++) next += per - (r < n_online ? (n_online - 1 - r) / world + 1 : 0);
    while ((int)n < per) groups[n++] = (uint8_t)next++;
    *n_groups = n;
    return RV_OK;
}

static int verify_sharded_impl(rv_comm* m, const rv_circuit* c, const uint8_t* proof, size_t proof_len, uint32_t flags, int* ok) {
    if (!m || !c || !proof || !ok || !verify_flags_ok(flags)) return RV_E_ARG;
    *ok = 0;
    rv_ctx* ctx = m->ctx;
    if (c->ctx != ctx) return RV_E_ARG;
    // ---- everything that can reject the proof without the GPU, before the collective: every rank sees the same bytes, so every
    //      rank returns here with the same answer and none is left waiting in the all-gather
    if (32 % m->world) return RV_E_ARG;  // (rv_comm_create takes any world; the verifier deals whole groups)
    Parsed P;
    int rc = parse_proof(proof, proof_len, P);
    if (rc) return rc;
    if (!format_ok(P)) return RV_OK;  // as rv_verify_ex: `false`, not an error
    if ((rc = check_records_range(P, 0, RV_TOTAL_REPS))) return rc;
    // ---- this rank's groups
    uint8_t groups[32];
    uint32_t n_groups = 0;
    if ((rc = rv_verify_partition(m->world, m->rank, groups, &n_groups))) return rc;
    const size_t part = (size_t)n_groups * 8 * 32 + VERIFY_TRAILER;
    std::vector<uint8_t> mine(part, 0);
    int zc = 1;
    if ((rc = verify_groups_impl(ctx, c, proof, proof_len, groups, n_groups, mine.data(), &zc))) return rc;
    mine[(size_t)n_groups * 8 * 32] = zc ? 1 : 0;
    // ---- the one collective, on the library's stream
    HIPCHK(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    std::vector<uint8_t> all(part * (size_t)m->world);
    HIPCHK(hipMemcpyAsync(m->d_vmine, mine.data(), part, hipMemcpyHostToDevice, st));
    if (m->world > 1) {
        if (rccl()->AllGather(m->d_vmine, m->d_vall, part, NCCL_UINT8, m->comm, st) != 0) return nccl_fail(1, "ncclAllGather");
    } else {
        HIPCHK(hipMemcpyAsync(m->d_vall, m->d_vmine, part, hipMemcpyDeviceToDevice, st));
    }
    HIPCHK(hipMemcpyAsync(all.data(), m->d_vall, all.size(), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    // ---- the digests back in slot order, the flags ANDed, and the decision on the host (one BLAKE3 over 8 KiB)
    std::vector<uint8_t> dig((size_t)RV_TOTAL_REPS * 32);
    int zc_all = 1;
    for (int r = 0; r < m->world; r++) {
        uint8_t g[32];
        uint32_t n = 0;
        if ((rc = rv_verify_partition(m->world, r, g, &n))) return rc;
        const uint8_t* at = all.data() + (size_t)r * part;
        for (uint32_t k = 0; k < n; k++) memcpy(dig.data() + (size_t)g[k] * 8 * 32, at + (size_t)k * 8 * 32, 8 * 32);
        if (!at[(size_t)n * 8 * 32]) zc_all = 0;
    }
    return rv_verify_finish_impl(proof, proof_len, dig.data(), flags, zc_all, ok);
}

extern "C" int rv_verify_sharded(rv_comm* m, const rv_circuit* c, const uint8_t* proof, size_t proof_len, uint32_t flags, int* ok) {
    return guarded([&] { return verify_sharded_impl(m, c, proof, proof_len, flags, ok); });
}

// one process, n GPUs: a host thread per rank runs rv_verify_sharded; every rank must come to the same (rc, ok)
extern "C" int rv_verify_multi(rv_comm* const* comms, const rv_circuit* const* circuits, int n, const uint8_t* proof, size_t proof_len,
                               uint32_t flags, int* ok) {
    if (!comms || !circuits || n < 1 || !proof || !ok) return RV_E_ARG;
    *ok = 0;
    std::vector<int> rcs((size_t)n, RV_OK), oks((size_t)n, 0);
    std::vector<std::string> errs((size_t)n);
    auto run = [&](int i) {
        rcs[(size_t)i] = rv_verify_sharded(comms[i], circuits[i], proof, proof_len, flags, &oks[(size_t)i]);
        if (rcs[(size_t)i]) errs[(size_t)i] = g_last_error;
    };
    std::vector<std::thread> th;
    for (int i = 1; i < n; i++) th.emplace_back(run, i);
    run(0);
    for (auto& t : th) t.join();
    for (int i = 1; i < n; i++)
        if (rcs[(size_t)i] != rcs[0] || oks[(size_t)i] != oks[0]) {
            g_last_error = "rv_verify_multi: rank " + std::to_string(i) + " answered (" + std::to_string(rcs[(size_t)i]) + ", " +
                           std::to_string(oks[(size_t)i]) + "), rank 0 (" + std::to_string(rcs[0]) + ", " + std::to_string(oks[0]) + ")";
            return RV_E_DEVICE;
        }
    if (rcs[0]) g_last_error = errs[0];
    *ok = oks[0];
    return rcs[0];
}
