// The pruning kernels as plain CPU loops (reverie_amd/csrc/prune_dev.hip), on the per-record code they share with the host function
// (reverie_amd/csrc/prune.h), in a stand-alone program for -fsanitize=address,undefined (tests/test_prune_host.py builds it with
// prune.cpp).  Every buffer is a heap block of exactly its bytes, so a read or a store one byte outside is reported.
//
//   prune_model [--max-rounds N] FILE...
// FILE (tests/test_prune_host.py: to_file): five u64 -- ops, z64_wires, gf2_wires, GF(2) outputs, Z64 outputs -- then the records and
// the two output lists (u32 each).
// For every file: rv_ops_prune's answer, then the device's order of work -- the counts in force and the checks, the sorted
// (index, op) pairs per domain, the searches, the reader counts, the queue peeled layer by layer (wavefront by wavefront and read by
// read, the solo loop and the wide rounds told apart as the kernels tell them), the keep flags' exclusive sum, and the emit tile by
// tile: the LDS image, the aligned 16-byte chunks and the 8-byte end pieces, into a 16-byte aligned buffer and into one 8 bytes off
// -- whose code, records, old_index and info must be rv_ops_prune's.  One line per file: "name code n_kept layers solo wide digest";
// the last line is "bad N" (N: the disagreements).  With --max-rounds the peeling stops as the device call does and the line ends in
// "fallback".
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <numeric>
#include <string>
#include <vector>

#include "prune.h"

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

constexpr uint32_t WG = 256, WAVE = 64, SOLO_LIMIT = 1024;  // prune_dev.h: PRUNE_WG, the wavefront, PRUNE_SOLO_LIMIT

static uint64_t fnv(const void* p, size_t n) {
    uint64_t h = 1469598103934665603ull;
    for (size_t i = 0; i < n; i++) h = (h ^ ((const uint8_t*)p)[i]) * 1099511628211ull;
    return h;
}

struct Writers {
    const uint32_t *sk[2], *sv[2];
    uint32_t nd[2];
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

// peel() of one wavefront whose lane l holds queue entry at[l] (have[l]: it holds one)
static void peel_wave(const bool have[WAVE], const uint32_t at[WAVE], const Exact<rv_op>& ops, const Writers& w, Exact<uint32_t>& cnt, Exact<uint32_t>& keep,
                      Exact<uint32_t>& queue, uint32_t& tail) {
    uint32_t i[WAVE] = {}, r[WAVE] = {}, rmax = 0;
    for (uint32_t l = 0; l < WAVE; l++)
        if (have[l]) {
            i[l] = queue[at[l]];
            keep[i[l]] = 0;
            r[l] = pr_n_reads(ops[i[l]]);
            rmax = std::max(rmax, r[l]);
        }
    for (uint32_t k = 0; k < rmax; k++) {
        bool freed[WAVE] = {};
        uint32_t v[WAVE] = {};
        for (uint32_t l = 0; l < WAVE; l++) {
            if (k >= r[l]) continue;
            const rv_op& op = ops[i[l]];
            const int rd = pr_read_dom(op);
            v[l] = pr_value_read(w.sk[rd], w.sv[rd], w.nd[rd], pr_read(op, k), i[l]);
            if (v[l] != PR_NONE && cnt[v[l]]-- == 1u) freed[l] = !pr_root(ops[v[l]]);
        }
        q_append(freed, v, queue, tail);
    }
}

static void run(const char* path, uint32_t max_rounds) {
    FILE* f = fopen(path, "rb");
    uint64_t h[5];
    if (!f || fread(h, 1, sizeof h, f) != sizeof h) {
        EXPECT(!"the file opens and has a header");
        if (f) fclose(f);
        return;
    }
    const size_t n = (size_t)h[0];
    const uint64_t z64_wires = h[1], gf2_wires = h[2];
    Exact<rv_op> ops(n);
    Exact<uint32_t> og((size_t)h[3]), oz((size_t)h[4]);
    bool ok = (!n || fread(ops.p, 24, n, f) == n) && (!og.n || fread(og.p, 4, og.n, f) == og.n) && (!oz.n || fread(oz.p, 4, oz.n, f) == oz.n);
    fclose(f);
    EXPECT(ok);
    if (!ok) return;
    const Exact<uint32_t>* outs[2] = {&og, &oz};
    const char* name = strrchr(path, '/') ? strrchr(path, '/') + 1 : path;

    // the host function: counting call, then the full one
    size_t want_kept = 0;
    rv_prune_info want = {}, counted = {};
    const int want_rc = rv_ops_prune(n ? ops.p : nullptr, n, z64_wires, gf2_wires, og.n ? og.p : nullptr, og.n, oz.n ? oz.p : nullptr, oz.n, nullptr, 0,
                                     &want_kept, nullptr, &counted);
    Exact<rv_op> want_out(want_rc ? 0 : want_kept);
    Exact<uint32_t> want_old(want_rc ? 0 : want_kept);
    if (!want_rc) {
        size_t kept2 = 0;
        EXPECT(rv_ops_prune(n ? ops.p : nullptr, n, z64_wires, gf2_wires, og.n ? og.p : nullptr, og.n, oz.n ? oz.p : nullptr, oz.n, want_out.p, want_kept,
                            &kept2, want_old.p, &want) == RV_OK);
        EXPECT(kept2 == want_kept && memcmp(&want, &counted, sizeof want) == 0);
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
    int rc = err != ~0ull ? (int)(err & 0xFF) : RV_OK;
    const uint64_t W[2] = {std::max<uint64_t>(gf2_wires, hg), std::max<uint64_t>(z64_wires, hz)};
    if (!rc)
        for (int d = 0; d < 2; d++)
            for (size_t k = 0; k < outs[d]->n; k++)
                if ((*outs[d])[k] >= W[d]) rc = RV_E_ARG;
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
        std::vector<uint32_t> order(n);
        std::iota(order.begin(), order.end(), 0u);
        std::vector<uint32_t> key(n);
        for (size_t i = 0; i < n; i++) key[i] = pr_def(ops[i]) == d ? ops[i].dst : (uint32_t)W[d];
        std::stable_sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) { return key[a] < key[b]; });
        sk[d] = new Exact<uint32_t>(n), sv[d] = new Exact<uint32_t>(n);
        for (size_t i = 0; i < n; i++) (*sk[d])[i] = key[order[i]], (*sv[d])[i] = order[i];
        w.sk[d] = sk[d]->p, w.sv[d] = sv[d]->p;
    }

    // step 3: the reader counts
    Exact<uint32_t> cnt(n), keep(n), queue(n);
    for (size_t i = 0; i < n; i++) {
        keep[i] = 1;
        const uint32_t r = pr_n_reads(ops[i]);
        const int rd = pr_read_dom(ops[i]);
        for (uint32_t k = 0; k < r; k++) {
            const uint32_t v = pr_value_read(w.sk[rd], w.sv[rd], w.nd[rd], pr_read(ops[i], k), (uint32_t)i);
            if (v != PR_NONE) cnt[v]++;
        }
    }
    for (int d = 0; d < 2; d++)
        for (size_t k = 0; k < outs[d]->n && w.nd[d]; k++) {
            const uint32_t v = pr_value_read(w.sk[d], w.sv[d], w.nd[d], (*outs[d])[k], PR_NONE);
            if (v != PR_NONE) cnt[v]++;
        }

    // step 4: the first frontier, wavefront by wavefront; then the layers
    uint32_t lo = 0, hi = 0, tail = 0, rounds = 0, solo = 0, wide = 0;
    for (size_t base = 0; base < n; base += WAVE) {
        bool dead[WAVE] = {};
        uint32_t idx[WAVE] = {};
        for (uint32_t l = 0; l < WAVE && base + l < n; l++) {
            const rv_op& op = ops[base + l];
            dead[l] = pr_def(op) >= 0 && !pr_root(op) && cnt[base + l] == 0;
            idx[l] = (uint32_t)(base + l);
        }
        q_append(dead, idx, queue, tail);
    }
    hi = tail;
    bool fallback = false;
    while (hi != lo) {
        if (rounds >= max_rounds) {
            fallback = true;
            break;
        }
        const bool is_solo = hi - lo <= SOLO_LIMIT;
        // (the solo kernel walks whole strides of its one workgroup; the wide kernel's workgroups take a stride each: the same walk)
        for (uint32_t base = lo; base < hi; base += WG)
            for (uint32_t wv = 0; wv < WG / WAVE; wv++) {
                bool have[WAVE] = {};
                uint32_t at[WAVE] = {};
                for (uint32_t l = 0; l < WAVE; l++) at[l] = base + wv * WAVE + l, have[l] = at[l] < hi;
                peel_wave(have, at, ops, w, cnt, keep, queue, tail);
            }
        rounds++, (is_solo ? solo : wide)++;
        lo = hi, hi = tail;
    }
    if (fallback) {
        printf("%s 0 %zu %u %u %u fallback\n", name, want_kept, rounds, solo, wide);
        for (int d = 0; d < 2; d++) delete sk[d], delete sv[d];
        return;
    }
    const size_t n_kept = n - tail;
    EXPECT(n_kept == want_kept);

    // step 5: the exclusive sum, the class counts, the tiles
    Exact<uint32_t> pos(n);
    uint32_t run_sum = 0;
    for (size_t i = 0; i < n; i++) pos[i] = run_sum, run_sum += keep[i];
    EXPECT(run_sum == n_kept);
    rv_prune_info got = {};
    got.n_kept = n_kept, got.n_dropped = n - n_kept;
    uint64_t* cls = &got.dropped_gf2_mul;
    for (size_t i = 0; i < n; i++) {
        if (!keep[i]) cls[pr_class(ops[i])]++;
        else if (pr_is_input(ops[i]) && cnt[i] == 0) cls[PR_C_INPUT_G + pr_def(ops[i])]++;
    }
    EXPECT(memcmp(&got, &want, sizeof got) == 0);
    uint64_t digest = 0;
    for (uint32_t off = 0; off <= 8 && n_kept == want_kept; off += 8) {  // d_out 16-byte aligned, and 8 bytes off
        Exact<uint8_t> room(n_kept * 24 + off);  // (malloc's blocks are 16-byte aligned)
        memset(room.p, 0xA5, room.n);
        uint8_t* out = room.p + off;
        Exact<uint32_t> old(n_kept);
        Exact<uint8_t> raw(PR_IMAGE);
        for (size_t t0 = 0; t0 < n; t0 += PRUNE_TILE) {
            const uint32_t mine = (uint32_t)std::min<size_t>(PRUNE_TILE, n - t0);
            const uint32_t first = pos[t0], kept_here = pos[t0 + mine - 1] + keep[t0 + mine - 1] - first;
            const uint32_t sh = pr_image_shift((uint64_t)(uintptr_t)out, first);
            for (uint32_t t = 0; t < mine; t++) {
                if (!keep[t0 + t]) continue;
                const uint32_t at = pos[t0 + t];
                memcpy(raw.p + sh + (at - first) * 24, &ops[t0 + t], 24);
                old[at] = (uint32_t)(t0 + t);
            }
            const uint32_t span = sh + kept_here * 24;
            uint8_t* base = out + (uint64_t)first * 24 - sh;
            EXPECT(((uintptr_t)base & 15u) == 0);
            for (uint32_t c = 0; c < span; c += 16) {
                const uint32_t kind = pr_chunk(c, sh, span);
                if (kind == 3) memcpy(base + c, raw.p + c, 16);
                else if (kind == 1) memcpy(base + c, raw.p + c, 8);
                else if (kind == 2) memcpy(base + c + 8, raw.p + c + 8, 8);
            }
        }
        for (uint32_t k = 0; k < off; k++) EXPECT(room[k] == 0xA5);
        EXPECT(n_kept == 0 || memcmp(out, want_out.p, n_kept * 24) == 0);
        EXPECT(n_kept == 0 || memcmp(old.p, want_old.p, n_kept * 4) == 0);
        digest = fnv(out, n_kept * 24);
    }
    printf("%s 0 %zu %u %u %u %016llx\n", name, n_kept, rounds, solo, wide, (unsigned long long)digest);
    for (int d = 0; d < 2; d++) delete sk[d], delete sv[d];
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
