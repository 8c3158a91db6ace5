// The folding kernels as plain CPU loops (reverie_amd/csrc/fold_dev.hip), on the per-record code they share with the host function
// (reverie_amd/csrc/fold.h), in a stand-alone program for -fsanitize=address,undefined (tests/test_fold_host.py builds it with
// fold.cpp).  Every buffer is a heap block of exactly its bytes, so a read or a store one byte outside is reported.
//
//   fold_model [--max-rounds N] FILE...
// FILE (tests/test_fold_host.py: to_file): three u64 -- ops, z64_wires, gf2_wires -- then the records.
// For every file: rv_ops_fold's answer, then the device's order of work -- the counts in force and the checks, the sorted
// (index, op) pairs per domain, the seed step wavefront by wavefront, the reader pairs at the exclusive sum of pending, sorted by
// producer, and their offsets, the queue stepped layer by layer (wavefront by wavefront and reader by reader, the solo loop and the
// wide rounds told apart as the kernels tell them), and the rewrite tile by tile: the LDS image, the aligned 16-byte chunks and the
// 8-byte end pieces, into a 16-byte aligned buffer and into one 8 bytes off -- whose code, records and info must be rv_ops_fold's.
// One line per file: "name code n_known layers solo wide digest"; the last line is "bad N" (N: the disagreements).  With
// --max-rounds the propagation stops as the device call does and the line ends in "fallback".
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <numeric>
#include <vector>

#include "fold.h"

using namespace rv;

static int g_bad = 0;
static const char* g_name = "";
#define EXPECT(x)                                                                \
    do {                                                                         \
        if (!(x)) {                                                              \
            g_bad++;                                                             \
            fprintf(stderr, "%s:%d: %s (%s)\n", __FILE__, __LINE__, #x, g_name); \
        }                                                                        \
    } while (0)

// a heap block of exactly n elements (n == 0: one that must not be touched at all)
template <class T>
struct Exact {
    T* p;
    size_t n;
    explicit Exact(size_t n_) : p((T*)malloc(n_ ? n_ * sizeof(T) : 1)), n(n_) {
        if (n) memset((void*)p, 0, n * sizeof(T));
    }
    ~Exact() { free(p); }
    Exact(const Exact&) = delete;
    T& operator[](size_t i) const { return p[i]; }
};

constexpr uint32_t WG = 256, WAVE = 64, SOLO_LIMIT = 1024;  // fold_dev.h: FOLD_WG, the wavefront, FOLD_SOLO_LIMIT

static uint64_t fnv(const void* p, size_t n) {
    uint64_t h = 1469598103934665603ull;
    for (size_t i = 0; i < n; i++) h = (h ^ ((const uint8_t*)p)[i]) * 1099511628211ull;
    return h;
}

struct Writers {
    const uint32_t *sk[2], *sv[2];
    uint32_t nd[2];
};
struct Fold {
    Exact<uint32_t>&pa, &pb, &pending, &known;
    Exact<uint64_t>& val;
};

// q_append of one wavefront: the lanes that have something take consecutive places behind the tail
static void q_append(const bool have[WAVE], const uint32_t v[WAVE], Exact<uint32_t>& queue, uint32_t& tail) {
    uint32_t count = 0;
    for (uint32_t l = 0; l < WAVE; l++) count += have[l];
    if (!count) return;
    uint32_t base = tail, rank = 0;
    tail += count;
    for (uint32_t l = 0; l < WAVE; l++)
        if (have[l]) queue[base + rank++] = v[l];
}

static uint64_t value_of(const rv_op& op, uint32_t r, const Writers& w, const Fold& f) {
    if (op.domain == RV_DOM_B2A) {
        uint64_t acc = 0;
        for (uint32_t k = 0; k < 64; k++) {
            const uint32_t p = pr_value_read(w.sk[PR_G], w.sv[PR_G], w.nd[PR_G], op.a + k, r);
            acc |= fd_b2a_bit(k, p == PR_NONE ? 0ull : f.val[p]);
        }
        return acc;
    }
    const uint32_t pa = f.pa[r], pb = f.pb[r];
    const uint64_t v[2] = {pa == PR_NONE ? 0ull : f.val[pa], pb == PR_NONE ? 0ull : f.val[pb]};
    return fd_eval(op, v);
}

// spread() of one wavefront whose lane l holds queue entry at[l] (have[l]: it holds one).  The values a layer stores are read by
// the next layer only: they go into `later` and are stored when the layer is done, so that a read of one inside the layer would show.
struct Stored {
    uint32_t op;
    uint64_t val;
};
static void spread_wave(const bool have[WAVE], const uint32_t at[WAVE], const Exact<rv_op>& ops, const Writers& w, const Fold& f, const Exact<uint32_t>& rk,
                        const Exact<uint32_t>& rv_, const Exact<uint32_t>& off, Exact<uint32_t>& queue, uint32_t& tail, std::vector<Stored>& later) {
    uint32_t p[WAVE] = {}, j[WAVE] = {};
    uint64_t pval[WAVE] = {};
    for (uint32_t l = 0; l < WAVE; l++)
        if (have[l]) p[l] = queue[at[l]], j[l] = off[p[l]], pval[l] = f.val[p[l]];
    for (;; ) {
        bool live[WAVE] = {}, any = false, claimed[WAVE] = {};
        uint32_t r[WAVE] = {};
        for (uint32_t l = 0; l < WAVE; l++) any |= live[l] = have[l] && j[l] < rk.n && rk[j[l]] == p[l];
        if (!any) break;
        for (uint32_t l = 0; l < WAVE; l++) {
            if (!live[l]) continue;
            r[l] = rv_[j[l]];
            const rv_op& op = ops[r[l]];
            bool mine = false;
            uint64_t value = 0;
            if (fd_zero_kills(op) && pval[l] == 0) mine = true;
            else if (f.pending[r[l]]-- == 1u) mine = true, value = value_of(op, r[l], w, f);
            if (mine && f.known[r[l]] == 0) f.known[r[l]] = 1, later.push_back({r[l], value}), claimed[l] = true;
        }
        q_append(claimed, r, queue, tail);
        for (uint32_t l = 0; l < WAVE; l++) j[l]++;
    }
}

static void run(const char* path, uint32_t max_rounds) {
    FILE* fp = fopen(path, "rb");
    uint64_t h[3];
    if (!fp || fread(h, 1, sizeof h, fp) != sizeof h) {
        EXPECT(!"the file opens and has a header");
        if (fp) fclose(fp);
        return;
    }
    const size_t n = (size_t)h[0];
    const uint64_t z64_wires = h[1], gf2_wires = h[2];
    Exact<rv_op> ops(n);
    const bool ok = !n || fread(ops.p, 24, n, fp) == n;
    fclose(fp);
    EXPECT(ok);
    if (!ok) return;
    const char* name = strrchr(path, '/') ? strrchr(path, '/') + 1 : path;

    // the host function: counting call, the full one, and in place
    rv_fold_info want = {}, counted = {};
    const int want_rc = rv_ops_fold(n ? ops.p : nullptr, n, z64_wires, gf2_wires, nullptr, &counted);
    Exact<rv_op> want_out(want_rc ? 0 : n);
    if (!want_rc) {
        EXPECT(rv_ops_fold(n ? ops.p : nullptr, n, z64_wires, gf2_wires, n ? want_out.p : nullptr, &want) == RV_OK);
        EXPECT(memcmp(&want, &counted, sizeof want) == 0);
        Exact<rv_op> again(n);
        if (n) memcpy(again.p, ops.p, n * 24);
        EXPECT(rv_ops_fold(n ? again.p : nullptr, n, z64_wires, gf2_wires, n ? again.p : nullptr, nullptr) == RV_OK);
        EXPECT(!n || memcmp(again.p, want_out.p, n * 24) == 0);
    }

    // step 1: the counts in force (an exclusive max-scan of the hints), the checks, the defining ops per domain
    Exact<uint32_t> cz(n), cg(n);
    uint32_t hz = 0, hg = 0;
    for (size_t i = 0; i < n; i++) {
        cz[i] = hz, cg[i] = hg;
        if (ops[i].domain == RV_DOM_SIZEHINT) hz = std::max(hz, ops[i].a), hg = std::max(hg, ops[i].b);
    }
    uint64_t err = ~0ull;
    uint32_t nd[2] = {0, 0};
    for (size_t i = 0; i < n; i++) {
        const int rc = pr_check(ops[i], std::max<uint64_t>(z64_wires, cz[i]), std::max<uint64_t>(gf2_wires, cg[i]));
        if (rc) err = std::min<uint64_t>(err, (uint64_t)i << 8 | (uint64_t)rc);
        else if (pr_def(ops[i]) >= 0) nd[pr_def(ops[i])]++;
    }
    const int rc = err != ~0ull ? (int)(err & 0xFF) : RV_OK;
    const uint64_t W[2] = {std::max<uint64_t>(gf2_wires, hg), std::max<uint64_t>(z64_wires, hz)};
    EXPECT(rc == want_rc);
    if (rc || want_rc) {
        printf("%s %d 0 0 0 0 0\n", name, rc);
        return;
    }

    // step 2: per domain with a defining op, the (index, op) pairs sorted by index (stable)
    Exact<uint32_t>*sk[2] = {nullptr, nullptr}, *sv[2] = {nullptr, nullptr};
    Writers w = {};
    for (int d = 0; d < 2; d++) {
        w.nd[d] = nd[d];
        if (!nd[d]) continue;
        std::vector<uint32_t> order(n), key(n);
        std::iota(order.begin(), order.end(), 0u);
        for (size_t i = 0; i < n; i++) key[i] = pr_def(ops[i]) == d ? ops[i].dst : (uint32_t)W[d];
        std::stable_sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) { return key[a] < key[b]; });
        sk[d] = new Exact<uint32_t>(n), sv[d] = new Exact<uint32_t>(n);
        for (size_t i = 0; i < n; i++) (*sk[d])[i] = key[order[i]], (*sv[d])[i] = order[i];
        w.sk[d] = sk[d]->p, w.sv[d] = sv[d]->p;
    }
    struct Free {
        Exact<uint32_t>**a, **b;
        ~Free() {
            for (int d = 0; d < 2; d++) delete a[d], delete b[d];
        }
    } free_pairs{sk, sv};

    // step 3: the seed, wavefront by wavefront
    Exact<uint32_t> pa(n), pb(n), pending(n), known(n), queue(n);
    Exact<uint64_t> val(n);
    const Fold f = {pa, pb, pending, known, val};
    uint32_t lo = 0, hi = 0, tail = 0, rounds = 0, solo = 0, wide = 0;
    uint64_t n_pairs = 0;
    bool any_unwritten = false;
    for (size_t base = 0; base < n; base += WAVE) {
        bool kn[WAVE] = {};
        uint32_t idx[WAVE] = {};
        for (uint32_t l = 0; l < WAVE && base + l < n; l++) {
            const size_t i = base + l;
            const rv_op& op = ops[i];
            const uint32_t r = pr_n_reads(op);
            const int rd = pr_read_dom(op);
            uint32_t p[2] = {PR_NONE, PR_NONE}, have = 0;
            for (uint32_t k = 0; k < r; k++) {
                const uint32_t v = pr_value_read(w.sk[rd], w.sv[rd], w.nd[rd], pr_read(op, k), (uint32_t)i);
                if (v != PR_NONE) have++;
                if (k < 2 && op.domain != RV_DOM_B2A) p[k] = v;
            }
            any_unwritten |= have < r;
            uint64_t value = 0;
            uint32_t pend = 0;
            if (pr_def(op) >= 0) {
                if (op.domain == RV_DOM_B2A) {
                    kn[l] = have == 0;
                } else {
                    const bool uw[2] = {r > 0 && p[0] == PR_NONE, r > 1 && p[1] == PR_NONE};
                    const uint64_t zero[2] = {0, 0};
                    kn[l] = fd_seed(op, uw);
                    if (kn[l]) value = fd_eval(op, zero);
                }
                if (!kn[l]) pend = have;
            }
            pa[i] = p[0], pb[i] = p[1], pending[i] = pend, known[i] = kn[l], val[i] = value;
            n_pairs += pend;
            idx[l] = (uint32_t)i;
        }
        q_append(kn, idx, queue, tail);
    }
    hi = tail;
    if (!tail && !any_unwritten) {  // the list as it is
        EXPECT(want.n_rewritten == 0 && want.n_known == 0 && (!n || memcmp(ops.p, want_out.p, n * 24) == 0));
        printf("%s 0 0 0 0 0 %016llx\n", name, (unsigned long long)fnv(ops.p, n * 24));
        return;
    }

    bool fallback = false;
    if (tail) {
        // step 4: the pairs at the exclusive sum of pending, sorted by producer (stable), the offsets
        Exact<uint32_t> pos(n), pk(n_pairs), pv(n_pairs), rk(n_pairs), rv_(n_pairs), off(n);
        uint32_t sum = 0;
        for (size_t i = 0; i < n; i++) pos[i] = sum, sum += pending[i];
        EXPECT(sum == n_pairs);
        for (size_t i = 0; i < n; i++) {
            if (!pending[i]) continue;
            uint32_t at = pos[i];
            const rv_op& op = ops[i];
            if (op.domain == RV_DOM_B2A) {
                for (uint32_t k = 0; k < 64; k++) {
                    const uint32_t v = pr_value_read(w.sk[PR_G], w.sv[PR_G], w.nd[PR_G], op.a + k, (uint32_t)i);
                    if (v != PR_NONE) pk[at] = v, pv[at] = (uint32_t)i, at++;
                }
            } else {
                const uint32_t p[2] = {pa[i], pb[i]};
                for (int k = 0; k < 2; k++)
                    if (p[k] != PR_NONE) pk[at] = p[k], pv[at] = (uint32_t)i, at++;
            }
            EXPECT(at == pos[i] + pending[i]);
        }
        std::vector<uint32_t> order(n_pairs);
        std::iota(order.begin(), order.end(), 0u);
        std::stable_sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) { return pk[a] < pk[b]; });
        for (size_t j = 0; j < n_pairs; j++) rk[j] = pk[order[j]], rv_[j] = pv[order[j]];
        for (size_t j = 0; j < n_pairs; j++)
            if (j == 0 || rk[j - 1] != rk[j]) off[rk[j]] = (uint32_t)j;

        // step 5: the layers
        while (hi != lo) {
            if (rounds >= max_rounds) {
                fallback = true;
                break;
            }
            const bool is_solo = hi - lo <= SOLO_LIMIT;
            std::vector<Stored> later;
            // (the solo kernel walks whole strides of its one workgroup; the wide kernel's workgroups take a stride each: the same walk)
            for (uint32_t base = lo; base < hi; base += WG)
                for (uint32_t wv = 0; wv < WG / WAVE; wv++) {
                    bool have[WAVE] = {};
                    uint32_t at[WAVE] = {};
                    for (uint32_t l = 0; l < WAVE; l++) at[l] = base + wv * WAVE + l, have[l] = at[l] < hi;
                    spread_wave(have, at, ops, w, f, rk, rv_, off, queue, tail, later);
                }
            for (const Stored& s : later) val[s.op] = s.val;
            rounds++, (is_solo ? solo : wide)++;
            lo = hi, hi = tail;
        }
    }
    if (fallback) {
        printf("%s 0 %llu %u %u %u fallback\n", name, (unsigned long long)want.n_known, rounds, solo, wide);
        return;
    }
    EXPECT(tail == want.n_known);

    // step 6: the rewrite, tile by tile
    rv_fold_info got = {};
    got.n_ops = n, got.n_known = tail;
    uint64_t* cls = &got.gf2_mul_to_const;
    uint64_t digest = 0;
    for (uint32_t shift = 0; shift <= 8; shift += 8) {  // d_out 16-byte aligned, and 8 bytes off
        Exact<uint8_t> room(n * 24 + shift);            // (malloc's blocks are 16-byte aligned)
        memset(room.p, 0xA5, room.n);
        uint8_t* out = room.p + shift;
        Exact<uint8_t> raw(PR_IMAGE);
        for (size_t t0 = 0; t0 < n; t0 += FOLD_TILE) {
            const uint32_t mine = (uint32_t)std::min<size_t>(FOLD_TILE, n - t0);
            const uint32_t sh = pr_image_shift((uint64_t)(uintptr_t)out, t0);
            for (uint32_t t = 0; t < mine; t++) {
                const size_t i = t0 + t;
                const rv_op& op = ops[i];
                const uint32_t r = op.domain == RV_DOM_B2A ? 0u : pr_n_reads(op);
                const uint32_t p[2] = {pa[i], pb[i]};
                bool kn[2] = {false, false};
                uint64_t v[2] = {0, 0};
                for (uint32_t k = 0; k < r; k++) {
                    kn[k] = p[k] == PR_NONE || known[p[k]] != 0;
                    v[k] = (kn[k] && p[k] != PR_NONE) ? val[p[k]] : 0;
                }
                const rv_op now = fd_rewrite(op, known[i] != 0, val[i], kn, v);
                const int c = fd_class(op, now, kn, v);
                if (c >= 0 && shift == 0) cls[c]++;
                memcpy(raw.p + sh + t * 24, &now, 24);
            }
            const uint32_t span = sh + mine * 24;
            uint8_t* base = out + (uint64_t)t0 * 24 - sh;
            EXPECT(((uintptr_t)base & 15u) == 0);
            for (uint32_t c = 0; c < span; c += 16) {
                const uint32_t kind = pr_chunk(c, sh, span);
                if (kind == 3) memcpy(base + c, raw.p + c, 16);
                else if (kind == 1) memcpy(base + c, raw.p + c, 8);
                else if (kind == 2) memcpy(base + c + 8, raw.p + c + 8, 8);
            }
        }
        for (uint32_t k = 0; k < shift; k++) EXPECT(room[k] == 0xA5);
        EXPECT(n == 0 || memcmp(out, want_out.p, n * 24) == 0);
        digest = fnv(out, n * 24);
    }
    for (int c = 0; c < FD_REWRITTEN; c++) got.n_rewritten += cls[c];
    EXPECT(memcmp(&got, &want, sizeof got) == 0);
    printf("%s 0 %u %u %u %u %016llx\n", name, tail, rounds, solo, wide, (unsigned long long)digest);
}

int main(int argc, char** argv) {
    uint32_t max_rounds = 65536;
    for (int k = 1; k < argc; k++) {
        if (!strcmp(argv[k], "--max-rounds") && k + 1 < argc) {
            max_rounds = (uint32_t)strtoul(argv[++k], nullptr, 10);
            continue;
        }
        g_name = argv[k];
        run(argv[k], max_rounds);
    }
    printf("bad %d\n", g_bad);
    return g_bad ? 1 : 0;
}
