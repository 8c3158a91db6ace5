// The windowed folding kernels as plain CPU loops (reverie_amd/csrc/fold_win.hip, fold_dev_kernels.inc), on the per-record code they
// share with the host function (reverie_amd/csrc/fold.h), in a stand-alone program for -fsanitize=address,undefined
// (tests/test_fold_window_host.py builds it with fold.cpp).  Every buffer is a heap block of exactly its bytes, so a read or a store
// one byte outside is reported.
//
//   fold_window_model [--max-rounds N] FILE... | @LIST
// FILE (tests/test_fold_window_host.py: to_file): four u64 -- ops, z64_wires, gf2_wires, cuts -- then the cuts (u64), then the
// records.  LIST: a file of file names, one per line.
// For every file: rv_ops_fold_windows_host's answer, then the device's order of work window by window with the tables carried -- the
// counts in force and the checks, the tables grown (known 0), the sorted (index, op) pairs per domain, the seed step with its
// escaping reads taken from the tables, the reader pairs (a blocked Mul's pad pair among them), the layers, the changed flags, their
// exclusive sum and the scatter into a log that doubles, the rewrite tile by tile at the window's place in a 16-byte aligned output
// and in one 8 bytes off, and the last-writer table update -- and then a replay of the log (lower bound, scatter) over windows cut
// otherwise, from the last to the first.  Code, records, info and log must be the host call's.
// One line per file: "name code n_known layers n_log digest"; the last line is "bad N" (N: the disagreements).  With --max-rounds a
// window's propagation stops as the device feed does, the window is stepped by the host sweep with the tables, and the line ends in
// "fallback K" (K: such windows).
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <numeric>
#include <string>
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

constexpr uint32_t WG = 256, WAVE = 64;  // fold_dev.h: FOLD_WG, the wavefront

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
// the tables: blocks of exactly the counts in force
struct Carried {
    Exact<uint8_t>* K[2];
    Exact<uint64_t>* V[2];
};
static bool carried(const Carried& c, int d, uint32_t w, uint64_t* v) {
    *v = 0;
    if ((*c.K[d])[w] == 0) return false;
    *v = (*c.V[d])[w];
    return true;
}
// k_fw_fill behind a copy of what the tables held
static void grow(Carried& c, int d, uint64_t want) {
    const size_t had = c.K[d]->n;
    if (want <= had) return;
    Exact<uint8_t>* k = new Exact<uint8_t>(want);
    Exact<uint64_t>* v = new Exact<uint64_t>(want);
    if (had) memcpy(k->p, c.K[d]->p, had), memcpy(v->p, c.V[d]->p, had * 8);
    for (size_t i = had; i < want; i++) (*k)[i] = 1, (*v)[i] = 0;
    delete c.K[d], delete c.V[d];
    c.K[d] = k, c.V[d] = v;
}

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

static uint64_t value_of(const rv_op& op, uint32_t r, const Writers& w, const Fold& f, const Carried& c) {
    uint64_t cv;
    if (op.domain == RV_DOM_B2A) {
        uint64_t acc = 0;
        for (uint32_t k = 0; k < 64; k++) {
            const uint32_t p = pr_value_read(w.sk[PR_G], w.sv[PR_G], w.nd[PR_G], op.a + k, r);
            acc |= fd_b2a_bit(k, p == PR_NONE ? (carried(c, PR_G, op.a + k, &cv), cv) : f.val[p]);
        }
        return acc;
    }
    const uint32_t pa = f.pa[r], pb = f.pb[r], nr = pr_n_reads(op);
    const int rd = pr_read_dom(op);
    uint64_t v[2] = {0, 0};
    if (nr > 0) v[0] = pa == PR_NONE ? (carried(c, rd, op.a, &cv), cv) : f.val[pa];
    if (nr > 1) v[1] = pb == PR_NONE ? (carried(c, rd, op.b, &cv), cv) : f.val[pb];
    return fd_eval(op, v);
}

// spread() of one wavefront whose lane l holds queue entry at[l] (have[l]: it holds one).  The values a layer stores are read by
// the next layer only: they go into `later` and are stored when the layer is done, so that a read of one inside the layer would show.
struct Stored {
    uint32_t op;
    uint64_t val;
};
static void spread_wave(const bool have[WAVE], const uint32_t at[WAVE], const rv_op* ops, uint32_t n, const Writers& w, const Fold& f, const Carried& c,
                        const Exact<uint32_t>& rk, const Exact<uint32_t>& rv_, const Exact<uint32_t>& off, Exact<uint32_t>& queue, uint32_t& tail,
                        std::vector<Stored>& later) {
    uint32_t p[WAVE] = {}, j[WAVE] = {};
    uint64_t pval[WAVE] = {};
    for (uint32_t l = 0; l < WAVE; l++)
        if (have[l]) p[l] = queue[at[l]], j[l] = off[p[l]], pval[l] = f.val[p[l]];
    for (;;) {
        bool live[WAVE] = {}, any = false, claimed[WAVE] = {};
        uint32_t r[WAVE] = {};
        for (uint32_t l = 0; l < WAVE; l++) any |= live[l] = have[l] && j[l] < rk.n && rk[j[l]] == p[l];
        if (!any) break;
        for (uint32_t l = 0; l < WAVE; l++) {
            if (!live[l]) continue;
            r[l] = rv_[j[l]];
            EXPECT(r[l] < n);
            const rv_op& op = ops[r[l]];
            bool mine = false;
            uint64_t value = 0;
            if (fd_zero_kills(op) && pval[l] == 0) mine = true;
            else if (f.pending[r[l]]-- == 1u) mine = true, value = value_of(op, r[l], w, f, c);
            if (mine && f.known[r[l]] == 0) f.known[r[l]] = 1, later.push_back({r[l], value}), claimed[l] = true;
        }
        q_append(claimed, r, queue, tail);
        for (uint32_t l = 0; l < WAVE; l++) j[l]++;
    }
}

// record i as the rewrite leaves it
static rv_op rewritten(const rv_op& op, size_t i, const Fold& f, const Carried& c, bool* kn, uint64_t* v) {
    const uint32_t r = op.domain == RV_DOM_B2A ? 0u : pr_n_reads(op);
    const int rd = pr_read_dom(op);
    const uint32_t p[2] = {f.pa[i], f.pb[i]};
    for (uint32_t k = 0; k < r; k++) {
        if (p[k] == PR_NONE) {
            kn[k] = carried(c, rd, pr_read(op, k), &v[k]);
        } else {
            kn[k] = f.known[p[k]] != 0u;
            v[k] = kn[k] ? f.val[p[k]] : 0ull;
        }
    }
    return fd_rewrite(op, f.known[i] != 0u, f.val[i], kn, v);
}

// the log: two blocks of exactly its capacity, doubled when full
struct Log {
    Exact<uint32_t>* ord = new Exact<uint32_t>(0);
    Exact<rv_op>* rec = new Exact<rv_op>(0);
    size_t n = 0;
    ~Log() { delete ord, delete rec; }
    void room(size_t more) {
        if (n + more <= ord->n) return;
        size_t cap = std::max<size_t>(ord->n, 4);
        while (cap < n + more) cap *= 2;
        Exact<uint32_t>* o = new Exact<uint32_t>(cap);
        Exact<rv_op>* r = new Exact<rv_op>(cap);
        if (n) memcpy(o->p, ord->p, n * 4), memcpy(r->p, rec->p, n * sizeof(rv_op));
        delete ord, delete rec;
        ord = o, rec = r;
    }
};

static void run(const char* path, uint32_t max_rounds) {
    FILE* fp = fopen(path, "rb");
    uint64_t h[4];
    if (!fp || fread(h, 1, sizeof h, fp) != sizeof h) {
        EXPECT(!"the file opens and has a header");
        if (fp) fclose(fp);
        return;
    }
    const size_t n = (size_t)h[0], n_cuts = (size_t)h[3];
    const uint64_t z64_wires = h[1], gf2_wires = h[2];
    Exact<uint64_t> cuts64(n_cuts);
    Exact<size_t> cuts(n_cuts);
    Exact<rv_op> ops(n);
    bool ok = !n_cuts || fread(cuts64.p, 8, n_cuts, fp) == n_cuts;
    ok = ok && (!n || fread(ops.p, 24, n, fp) == n);
    fclose(fp);
    EXPECT(ok);
    if (!ok) return;
    for (size_t k = 0; k < n_cuts; k++) cuts[k] = (size_t)cuts64[k];
    const char* name = strrchr(path, '/') ? strrchr(path, '/') + 1 : path;

    // the host function: counting call, the full one, in place
    rv_fold_info want = {}, counted = {};
    const int want_rc = rv_ops_fold_windows_host(n ? ops.p : nullptr, n, z64_wires, gf2_wires, n_cuts ? cuts.p : nullptr, n_cuts, nullptr, &counted);
    Exact<rv_op> want_out(want_rc ? 0 : n);
    if (!want_rc) {
        EXPECT(rv_ops_fold_windows_host(n ? ops.p : nullptr, n, z64_wires, gf2_wires, n_cuts ? cuts.p : nullptr, n_cuts, n ? want_out.p : nullptr, &want) == RV_OK);
        EXPECT(memcmp(&want, &counted, sizeof want) == 0);
        Exact<rv_op> again(n);
        if (n) memcpy(again.p, ops.p, n * 24);
        EXPECT(rv_ops_fold_windows_host(n ? again.p : nullptr, n, z64_wires, gf2_wires, n_cuts ? cuts.p : nullptr, n_cuts, n ? again.p : nullptr, nullptr) == RV_OK);
        EXPECT(!n || memcmp(again.p, want_out.p, n * 24) == 0);
        // and the whole-list call
        Exact<rv_op> whole(n);
        rv_fold_info wi = {};
        EXPECT(rv_ops_fold(n ? ops.p : nullptr, n, z64_wires, gf2_wires, n ? whole.p : nullptr, &wi) == RV_OK);
        EXPECT((!n || memcmp(whole.p, want_out.p, n * 24) == 0) && memcmp(&wi, &want, sizeof wi) == 0);
    }

    // the folder's state
    uint64_t W[2] = {gf2_wires, z64_wires};
    Carried c = {{new Exact<uint8_t>(0), new Exact<uint8_t>(0)}, {new Exact<uint64_t>(0), new Exact<uint64_t>(0)}};
    struct FreeTables {
        Carried& c;
        ~FreeTables() {
            for (int d = 0; d < 2; d++) delete c.K[d], delete c.V[d];
        }
    } free_tables{c};
    for (int d = 0; d < 2; d++) grow(c, d, W[d]);
    Log log;
    rv_fold_info got = {};
    got.n_ops = n;
    uint64_t* cls = &got.gf2_mul_to_const;
    uint32_t layers = 0, fallbacks = 0;
    int rc = RV_OK;
    // the two outputs: 16-byte aligned, and 8 bytes off (malloc's blocks are 16-byte aligned)
    Exact<uint8_t> room0(n * 24), room8(n * 24 + 8);
    memset(room0.p, 0xA5, room0.n), memset(room8.p, 0xA5, room8.n);
    uint8_t* outs[2] = {room0.p, room8.p + 8};

    size_t lo = 0;
    for (size_t wnd = 0; wnd <= n_cuts && rc == RV_OK; wnd++) {
        const size_t hi = wnd < n_cuts ? cuts[wnd] : n;
        const size_t m = hi - lo;
        const rv_op* wops = ops.p + lo;
        if (!m) continue;  // (a feed of 0 ops launches nothing)

        // step 1: the counts in force (an exclusive max-scan of the hints, seeded with the carried counts), the checks
        Exact<uint32_t> cz(m), cg(m);
        uint32_t hz = 0, hg = 0;
        for (size_t i = 0; i < m; i++) {
            cz[i] = hz, cg[i] = hg;
            if (wops[i].domain == RV_DOM_SIZEHINT) hz = std::max(hz, wops[i].a), hg = std::max(hg, wops[i].b);
        }
        uint64_t err = ~0ull;
        uint32_t nd[2] = {0, 0};
        for (size_t i = 0; i < m; i++) {
            const int e = pr_check(wops[i], std::max<uint64_t>(W[PR_Z], cz[i]), std::max<uint64_t>(W[PR_G], cg[i]));
            if (e) err = std::min<uint64_t>(err, (uint64_t)i << 8 | (uint64_t)e);
            else if (pr_def(wops[i]) >= 0) nd[pr_def(wops[i])]++;
        }
        if (err != ~0ull) {
            rc = (int)(err & 0xFF);  // (nothing is written for this feed)
            break;
        }
        W[PR_G] = std::max<uint64_t>(W[PR_G], hg), W[PR_Z] = std::max<uint64_t>(W[PR_Z], hz);
        for (int d = 0; d < 2; d++) grow(c, d, W[d]);

        // step 2: per domain with a defining op, the (index, op) pairs sorted by index (stable)
        Exact<uint32_t>*sk[2] = {nullptr, nullptr}, *sv[2] = {nullptr, nullptr};
        Writers w = {};
        for (int d = 0; d < 2; d++) {
            w.nd[d] = nd[d];
            if (!nd[d]) continue;
            std::vector<uint32_t> order(m), key(m);
            std::iota(order.begin(), order.end(), 0u);
            for (size_t i = 0; i < m; i++) key[i] = pr_def(wops[i]) == d ? wops[i].dst : (uint32_t)W[d];
            std::stable_sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) { return key[a] < key[b]; });
            sk[d] = new Exact<uint32_t>(m), sv[d] = new Exact<uint32_t>(m);
            for (size_t i = 0; i < m; i++) (*sk[d])[i] = key[order[i]], (*sv[d])[i] = order[i];
            w.sk[d] = sk[d]->p, w.sv[d] = sv[d]->p;
        }
        struct Free {
            Exact<uint32_t>**a, **b;
            ~Free() {
                for (int d = 0; d < 2; d++) delete a[d], delete b[d];
            }
        } free_pairs{sk, sv};

        // step 3: the seed, wavefront by wavefront, the escaping reads from the tables
        Exact<uint32_t> pa(m), pb(m), pending(m), known(m), queue(m);
        Exact<uint64_t> val(m);
        const Fold f = {pa, pb, pending, known, val};
        uint32_t qlo = 0, qhi = 0, tail = 0, rounds = 0;
        uint64_t n_pairs = 0;
        bool any_known_escape = false;
        for (size_t base = 0; base < m; base += WAVE) {
            bool kn_l[WAVE] = {};
            uint32_t idx[WAVE] = {};
            for (uint32_t l = 0; l < WAVE && base + l < m; l++) {
                const size_t i = base + l;
                const rv_op& op = wops[i];
                const uint32_t r = pr_n_reads(op);
                const int rd = pr_read_dom(op);
                uint32_t p[2] = {PR_NONE, PR_NONE}, have = 0;
                bool kn[2] = {false, false}, blocked = false;
                uint64_t ev[2] = {0, 0}, bits = 0;
                for (uint32_t k = 0; k < r; k++) {
                    const uint32_t v = pr_value_read(w.sk[rd], w.sv[rd], w.nd[rd], pr_read(op, k), (uint32_t)i);
                    if (v != PR_NONE) have++;
                    if (k < 2 && op.domain != RV_DOM_B2A) p[k] = v;
                    if (v == PR_NONE) {
                        uint64_t cv;
                        const bool ck = carried(c, rd, pr_read(op, k), &cv);
                        any_known_escape |= ck, blocked |= !ck;
                        if (op.domain == RV_DOM_B2A) bits |= fd_b2a_bit(k, cv);
                        else if (k < 2) kn[k] = ck, ev[k] = cv;
                    }
                }
                uint64_t value = 0;
                uint32_t pend = 0;
                if (pr_def(op) >= 0) {
                    if (op.domain == RV_DOM_B2A) {
                        kn_l[l] = have == 0 && !blocked;
                        if (kn_l[l]) value = bits;
                    } else {
                        kn_l[l] = fd_known(op, kn, ev);
                        if (kn_l[l]) value = fd_eval(op, ev);
                    }
                    if (!kn_l[l]) pend = !blocked ? have : (fd_zero_kills(op) && have) ? have + 1u : 0u;
                }
                pa[i] = p[0], pb[i] = p[1], pending[i] = pend, known[i] = kn_l[l], val[i] = value;
                n_pairs += pend;
                idx[l] = (uint32_t)i;
            }
            q_append(kn_l, idx, queue, tail);
        }
        qhi = tail;
        bool on_host = false;
        const bool copied = !tail && !any_known_escape;  // the records as they are; the tables are updated all the same
        if (tail) {
            // step 4: the pairs at the exclusive sum of pending, sorted by producer (stable), the offsets
            Exact<uint32_t> pos(m), pk(n_pairs), pv(n_pairs), rk(n_pairs), rv_(n_pairs), off(m);
            uint32_t sum = 0;
            for (size_t i = 0; i < m; i++) pos[i] = sum, sum += pending[i];
            EXPECT(sum == n_pairs);
            for (size_t i = 0; i < m; i++) {
                if (!pending[i]) continue;
                uint32_t at = pos[i];
                const rv_op& op = wops[i];
                if (op.domain == RV_DOM_B2A) {
                    for (uint32_t k = 0; k < 64; k++) {
                        const uint32_t v = pr_value_read(w.sk[PR_G], w.sv[PR_G], w.nd[PR_G], op.a + k, (uint32_t)i);
                        if (v != PR_NONE) pk[at] = v, pv[at] = (uint32_t)i, at++;
                    }
                } else {
                    const uint32_t p[2] = {pa[i], pb[i]};
                    for (int k = 0; k < 2; k++)
                        if (p[k] != PR_NONE) pk[at] = p[k], pv[at] = (uint32_t)i, at++;
                    if (at < pos[i] + pending[i]) pk[at] = (uint32_t)m, pv[at] = (uint32_t)i, at++;  // a blocked Mul's pad
                }
                EXPECT(at == pos[i] + pending[i]);
            }
            std::vector<uint32_t> order(n_pairs);
            std::iota(order.begin(), order.end(), 0u);
            std::stable_sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) { return pk[a] < pk[b]; });
            for (size_t j = 0; j < n_pairs; j++) rk[j] = pk[order[j]], rv_[j] = pv[order[j]];
            for (size_t j = 0; j < n_pairs; j++)
                if ((j == 0 || rk[j - 1] != rk[j]) && rk[j] < m) off[rk[j]] = (uint32_t)j;

            // step 5: the layers
            while (qhi != qlo) {
                if (rounds >= max_rounds) {
                    on_host = true;
                    break;
                }
                std::vector<Stored> later;
                for (uint32_t base = qlo; base < qhi; base += WG)
                    for (uint32_t wv = 0; wv < WG / WAVE; wv++) {
                        bool have[WAVE] = {};
                        uint32_t at[WAVE] = {};
                        for (uint32_t l = 0; l < WAVE; l++) at[l] = base + wv * WAVE + l, have[l] = at[l] < qhi;
                        spread_wave(have, at, wops, (uint32_t)m, w, f, c, rk, rv_, off, queue, tail, later);
                    }
                for (const Stored& s : later) val[s.op] = s.val;
                rounds++;
                qlo = qhi, qhi = tail;
            }
        }
        layers += rounds;
        if (on_host) {
            // the fall-back: the host sweep on the window with the tables, its records and log entries
            fallbacks++;
            Exact<rv_op> now(m);
            uint8_t* const K[2] = {c.K[PR_G]->p, c.K[PR_Z]->p};
            uint64_t* const V[2] = {c.V[PR_G]->p, c.V[PR_Z]->p};
            fold_window_dense(wops, m, K, V, now.p, cls, &got.n_known);
            for (size_t i = 0; i < m; i++)
                if (fd_changed(wops[i], now[i])) log.room(1), (*log.ord)[log.n] = (uint32_t)(lo + i), (*log.rec)[log.n] = now[i], log.n++;
            for (int s = 0; s < 2; s++) memcpy(outs[s] + lo * 24, now.p, m * 24);
            lo = hi;
            continue;
        }
        got.n_known += tail;

        if (copied) {
            for (int s = 0; s < 2; s++) memcpy(outs[s] + lo * 24, wops, m * 24);
        } else {
            // the log, before the rewrite: flags (in the queue's place), their exclusive sum (in pending's), the scatter
            uint32_t more = 0;
            for (size_t i = 0; i < m; i++) {
                bool kn[2] = {false, false};
                uint64_t v[2] = {0, 0};
                queue[i] = fd_changed(wops[i], rewritten(wops[i], i, f, c, kn, v)) ? 1u : 0u;
            }
            for (size_t i = 0; i < m; i++) pending[i] = more, more += queue[i];
            log.room(more);
            for (size_t i = 0; i < m; i++) {
                if (!queue[i]) continue;
                bool kn[2] = {false, false};
                uint64_t v[2] = {0, 0};
                (*log.ord)[log.n + pending[i]] = (uint32_t)(lo + i);
                (*log.rec)[log.n + pending[i]] = rewritten(wops[i], i, f, c, kn, v);
            }
            log.n += more;

            // step 6: the rewrite, tile by tile, at the window's place in both outputs
            for (int s = 0; s < 2; s++) {
                uint8_t* out = outs[s] + lo * 24;
                Exact<uint8_t> raw(PR_IMAGE);
                for (size_t t0 = 0; t0 < m; t0 += FOLD_TILE) {
                    const uint32_t mine = (uint32_t)std::min<size_t>(FOLD_TILE, m - t0);
                    const uint32_t sh = pr_image_shift((uint64_t)(uintptr_t)out, t0);
                    for (uint32_t t = 0; t < mine; t++) {
                        const size_t i = t0 + t;
                        bool kn[2] = {false, false};
                        uint64_t v[2] = {0, 0};
                        const rv_op now = rewritten(wops[i], i, f, c, kn, v);
                        const int cl = fd_class(wops[i], now, kn, v);
                        if (cl >= 0 && s == 0) cls[cl]++;
                        memcpy(raw.p + sh + t * 24, &now, 24);
                    }
                    const uint32_t span = sh + mine * 24;
                    uint8_t* base = out + (uint64_t)t0 * 24 - sh;
                    EXPECT(((uintptr_t)base & 15u) == 0);
                    for (uint32_t ch = 0; ch < span; ch += 16) {
                        const uint32_t kind = pr_chunk(ch, sh, span);
                        if (kind == 3) memcpy(base + ch, raw.p + ch, 16);
                        else if (kind == 1) memcpy(base + ch, raw.p + ch, 8);
                        else if (kind == 2) memcpy(base + ch + 8, raw.p + ch + 8, 8);
                    }
                }
            }
        }
        // the tables, after everything that read them: one pair per index stores
        for (int d = 0; d < 2; d++) {
            Exact<uint8_t> stored(W[d]);
            for (uint32_t j = 0; j < w.nd[d]; j++) {
                if (pr_run_last(w.sk[d], w.nd[d], j) && w.sk[d][j] < W[d]) EXPECT(stored[w.sk[d][j]]++ == 0);
                fd_table_update(w.sk[d], w.sv[d], w.nd[d], j, known.p, val.p, c.K[d]->p, c.V[d]->p, W[d]);
            }
        }
        lo = hi;
    }
    EXPECT(rc == want_rc);
    if (rc || want_rc) {
        printf("%s %d 0 0 0 0\n", name, rc);
        return;
    }
    for (int k = 0; k < FD_REWRITTEN; k++) got.n_rewritten += cls[k];
    EXPECT(memcmp(&got, &want, sizeof got) == 0);
    for (int s = 0; s < 2; s++) EXPECT(n == 0 || memcmp(outs[s], want_out.p, n * 24) == 0);
    for (uint32_t k = 0; k < 8; k++) EXPECT(room8[k] == 0xA5);
    EXPECT(log.n == want.n_rewritten);
    for (size_t j = 1; j < log.n; j++) EXPECT((*log.ord)[j - 1] < (*log.ord)[j]);

    // the replay: windows of 37 records from the last to the first, over copies of the source records
    Exact<rv_op> back(n);
    for (size_t end = n; end > 0;) {
        const size_t first = end > 37 ? end - 37 : 0, cnt = end - first;
        Exact<rv_op> piece(cnt);
        memcpy(piece.p, ops.p + first, cnt * 24);
        const uint32_t b0 = fd_log_lower_bound(log.ord->p, (uint32_t)log.n, first), b1 = fd_log_lower_bound(log.ord->p, (uint32_t)log.n, first + cnt);
        EXPECT(b0 <= b1 && b1 <= log.n);
        for (uint32_t j = b0; j < b1; j++) {
            const uint64_t o = (uint64_t)(*log.ord)[j] - first;
            EXPECT(o < cnt);
            if (o < cnt) piece[o] = (*log.rec)[j];
        }
        memcpy(back.p + first, piece.p, cnt * 24);
        end = first;
    }
    EXPECT(n == 0 || memcmp(back.p, want_out.p, n * 24) == 0);
    printf("%s 0 %llu %u %zu %016llx", name, (unsigned long long)got.n_known, layers, log.n, (unsigned long long)fnv(outs[0], n * 24));
    if (fallbacks) printf(" fallback %u", fallbacks);
    printf("\n");
}

int main(int argc, char** argv) {
    uint32_t max_rounds = 65536;
    std::vector<std::string> files;
    for (int k = 1; k < argc; k++) {
        if (!strcmp(argv[k], "--max-rounds") && k + 1 < argc) {
            max_rounds = (uint32_t)strtoul(argv[++k], nullptr, 10);
        } else if (argv[k][0] == '@') {
            FILE* fp = fopen(argv[k] + 1, "r");
            char line[4096];
            while (fp && fgets(line, sizeof line, fp)) {
                line[strcspn(line, "\r\n")] = 0;
                if (line[0]) files.push_back(line);
            }
            if (fp) fclose(fp);
        } else {
            files.push_back(argv[k]);
        }
    }
    for (const std::string& f : files) {
        g_name = f.c_str();
        run(f.c_str(), max_rounds);
    }
    printf("bad %d\n", g_bad);
    return g_bad ? 1 : 0;
}
