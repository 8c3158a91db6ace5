// The window step of the windowed pruning (reverie_amd/csrc/prune_win.hip) as plain CPU loops, on the per-record code it shares with
// the host function (reverie_amd/csrc/prune.h), in a stand-alone program for -fsanitize=address,undefined
// (tests/test_prune_window_host.py builds it).  Every buffer is a heap block of exactly its bytes, so a read or a store one byte
// outside is reported.
//
//   prune_window_model FILE...
// FILE (tests/test_prune_window_host.py: to_file): six u64 -- ops, z64_wires, gf2_wires, GF(2) outputs, Z64 outputs, cuts -- then the
// records, the two output lists (u32 each) and the cut positions (u64 each).  The list is a valid one.
// For every file the mark pass over the windows from the last to the first, twice: in the device's order of work (the sorted pairs
// of the window, the searches, the reader counts, the live-out, the peeling, kill, gen: pr_value_read, pr_live_out, pr_kill, pr_gen)
// and by the host's backward sweep (pr_window_sweep); both over needed tables of exactly the final wire counts.  The keep flags and
// the needed tables must agree after every window.  One line per file: "name layers flags" (flags: one 0 / 1 per op); the last line
// is "bad N" (N: the disagreements).
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <numeric>
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

// one window in the device's order; N[d]: W[d] bytes; keep: n bytes -> the layers peeled
static uint32_t device_step(const rv_op* ops, size_t n, uint8_t* const N[2], const uint64_t W[2], uint8_t* keep) {
    // the sorted (index, op) pairs per domain; nd: the defining ops
    Exact<uint32_t> sk0(n), sv0(n), sk1(n), sv1(n);
    Exact<uint32_t>* sk[2] = {&sk0, &sk1};
    Exact<uint32_t>* sv[2] = {&sv0, &sv1};
    uint32_t nd[2] = {0, 0};
    for (int d = 0; d < 2; d++) {
        std::vector<uint32_t> order(n), key(n);
        std::iota(order.begin(), order.end(), 0u);
        for (size_t i = 0; i < n; i++) key[i] = pr_def(ops[i]) == d ? ops[i].dst : (uint32_t)W[d], nd[d] += pr_def(ops[i]) == d;
        std::stable_sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) { return key[a] < key[b]; });
        for (size_t i = 0; i < n; i++) (*sk[d])[i] = key[order[i]], (*sv[d])[i] = order[i];
    }
    // the reader counts, then the live-out
    Exact<uint32_t> cnt(n), queue(n);
    for (size_t i = 0; i < n; i++) {
        keep[i] = 1;
        const uint32_t r = pr_n_reads(ops[i]);
        const int rd = pr_read_dom(ops[i]);
        for (uint32_t k = 0; k < r; k++) {
            const uint32_t v = pr_value_read(sk[rd]->p, sv[rd]->p, nd[rd], pr_read(ops[i], k), (uint32_t)i);
            if (v != PR_NONE) cnt[v]++;
        }
    }
    for (int d = 0; d < 2; d++)
        for (uint32_t j = 0; j < nd[d]; j++)
            if (pr_live_out(sk[d]->p, nd[d], j, N[d], W[d])) cnt[(*sv[d])[j]]++;
    // the peeling, layer by layer
    uint32_t lo = 0, hi = 0, tail = 0, layers = 0;
    for (size_t i = 0; i < n; i++)
        if (pr_def(ops[i]) >= 0 && !pr_root(ops[i]) && cnt[i] == 0) queue[tail++] = (uint32_t)i;
    hi = tail;
    while (hi != lo) {
        for (uint32_t at = lo; at < hi; at++) {
            const uint32_t i = queue[at];
            keep[i] = 0;
            const uint32_t r = pr_n_reads(ops[i]);
            const int rd = pr_read_dom(ops[i]);
            for (uint32_t k = 0; k < r; k++) {
                const uint32_t v = pr_value_read(sk[rd]->p, sv[rd]->p, nd[rd], pr_read(ops[i], k), i);
                if (v != PR_NONE && cnt[v]-- == 1u && !pr_root(ops[v])) queue[tail++] = v;
            }
        }
        layers++, lo = hi, hi = tail;
    }
    // kill, then gen
    for (int d = 0; d < 2; d++)
        for (uint32_t j = 0; j < nd[d]; j++) pr_kill(sk[d]->p, nd[d], j, N[d], W[d]);
    for (size_t i = 0; i < n; i++) {
        if (!keep[i]) continue;
        const uint32_t r = pr_n_reads(ops[i]);
        const int rd = pr_read_dom(ops[i]);
        for (uint32_t k = 0; k < r; k++) pr_gen(ops[i], (uint32_t)i, k, sk[rd]->p, sv[rd]->p, nd[rd], N[rd], W[rd]);
    }
    return layers;
}

static void run(const char* path) {
    FILE* f = fopen(path, "rb");
    uint64_t h[6];
    if (!f || fread(h, 1, sizeof h, f) != sizeof h) {
        EXPECT(!"the file opens and has a header");
        if (f) fclose(f);
        return;
    }
    const size_t n = (size_t)h[0];
    Exact<rv_op> ops(n);
    Exact<uint32_t> og((size_t)h[3]), oz((size_t)h[4]);
    Exact<uint64_t> cuts((size_t)h[5]);
    const bool ok = (!n || fread(ops.p, 24, n, f) == n) && (!og.n || fread(og.p, 4, og.n, f) == og.n) && (!oz.n || fread(oz.p, 4, oz.n, f) == oz.n) &&
                    (!cuts.n || fread(cuts.p, 8, cuts.n, f) == cuts.n);
    fclose(f);
    EXPECT(ok);
    if (!ok) return;
    const char* name = strrchr(path, '/') ? strrchr(path, '/') + 1 : path;
    uint64_t W[2] = {h[2], h[1]};
    for (size_t i = 0; i < n; i++)
        if (ops[i].domain == RV_DOM_SIZEHINT) W[PR_G] = std::max<uint64_t>(W[PR_G], ops[i].b), W[PR_Z] = std::max<uint64_t>(W[PR_Z], ops[i].a);

    // the needed tables of both forms, exactly the final counts long; 1 on the output indices
    Exact<uint8_t> dg((size_t)W[PR_G]), dz((size_t)W[PR_Z]), hg((size_t)W[PR_G]), hz((size_t)W[PR_Z]);
    for (size_t k = 0; k < og.n; k++) dg[og[k]] = hg[og[k]] = 1;
    for (size_t k = 0; k < oz.n; k++) dz[oz[k]] = hz[oz[k]] = 1;
    uint8_t* const N[2] = {dg.p, dz.p};
    PrDense need[2] = {{hg.p}, {hz.p}};
    Exact<uint8_t> keep_d(n), keep_h(n);
    uint64_t cls[PR_CLASSES] = {}, kept_h = 0;
    uint32_t layers = 0;
    for (size_t c = cuts.n + 1; c-- > 0;) {
        const size_t lo = c ? (size_t)cuts[c - 1] : 0, hi = c < cuts.n ? (size_t)cuts[c] : n;
        EXPECT(lo <= hi && hi <= n);
        if (lo > hi || hi > n) return;
        layers += device_step(ops.p + lo, hi - lo, N, W, keep_d.p + lo);
        kept_h += pr_window_sweep(ops.p + lo, hi - lo, need, keep_h.p + lo, cls);
        EXPECT(hi == lo || memcmp(keep_d.p + lo, keep_h.p + lo, hi - lo) == 0);
        EXPECT(!W[PR_G] || memcmp(dg.p, hg.p, (size_t)W[PR_G]) == 0);
        EXPECT(!W[PR_Z] || memcmp(dz.p, hz.p, (size_t)W[PR_Z]) == 0);
    }
    uint64_t kept_d = 0;
    for (size_t i = 0; i < n; i++) kept_d += keep_d[i];
    EXPECT(kept_d == kept_h);
    printf("%s %u ", name, layers);
    for (size_t i = 0; i < n; i++) putchar('0' + keep_d[i]);
    putchar('\n');
}

int main(int argc, char** argv) {
    for (int k = 1; k < argc; k++) {
        g_name = argv[k];
        run(argv[k]);
    }
    printf("bad %d\n", g_bad);
    return g_bad ? 1 : 0;
}
