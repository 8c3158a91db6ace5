// The linker's kernels as plain CPU loops (reverie_amd/csrc/link_dev.hip), on the per-record code they share with the host function
// (reverie_amd/csrc/link.h), in a stand-alone program for -fsanitize=address,undefined (tests/test_link_host.py builds it with
// link.cpp).  Every buffer is a heap block of exactly its bytes, so a read or a store one byte outside is reported.
//
//   link_model FILE... [--ranges FILE...]
// FILE (tests/link_cases.py: to_file): seven u64 -- blocks, instances, bindings, z64_base, gf2_base, head and tail records; per block
// three u64 (records, z64_wires, gf2_wires) and its records; block_of, bindings (u32 each); head; tail.
// For every file: rv_link's answer, then the plan's stages in the kernels' order of work -- judge, port scan, gather, prefix sums,
// binding check -- whose code and info must be rv_link's, then the emit kernel tile by tile and "thread" by "thread" -- the tile's
// first instance, the doubling search, the LDS image, the aligned chunks and the 8-byte end pieces -- for the whole list into a
// 16-byte aligned buffer and into one that is 8 bytes off, and behind --ranges for every (first, n).  One line per file:
// "name code n_ops digest", then "ranges name count"; the last line is "bad N" (N: the disagreements).
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <string>
#include <vector>

#include "link.h"

using namespace rv;

static int g_bad = 0;
#define EXPECT(x)                                                              \
    do {                                                                       \
        if (!(x)) {                                                            \
            g_bad++;                                                           \
            fprintf(stderr, "%s:%d: %s (%s)\n", __FILE__, __LINE__, #x, g_name); \
        }                                                                      \
    } while (0)
static const char* g_name = "";

// a heap block of exactly n elements (n == 0: one that must not be touched at all)
template <class T>
struct Exact {
    T* p;
    size_t n;
    explicit Exact(size_t n_) : p((T*)malloc(n_ ? n_ * sizeof(T) : 1)), n(n_) {
        if (n) memset(p, 0, n * sizeof(T));
    }
    ~Exact() { free(p); }
    Exact(const Exact&) = delete;
    T& operator[](size_t i) const { return p[i]; }
};

struct Case {
    std::vector<rv_link_block> blocks;
    std::vector<Exact<uint64_t>*> block_ops;
    Exact<uint32_t>*block_of = nullptr, *bindings = nullptr;
    Exact<uint64_t>*head = nullptr, *tail = nullptr;
    rv_link_desc d = {};
    ~Case() {
        for (auto* b : block_ops) delete b;
        delete block_of, delete bindings, delete head, delete tail;
    }
};

static bool read_exact(FILE* f, void* p, size_t bytes) { return bytes == 0 || fread(p, 1, bytes, f) == bytes; }

static bool load(const char* path, Case& c) {
    FILE* f = fopen(path, "rb");
    if (!f) return false;
    uint64_t h[7];
    bool ok = read_exact(f, h, sizeof h);
    for (uint64_t b = 0; ok && b < h[0]; b++) {
        uint64_t k[3];
        ok = read_exact(f, k, sizeof k);
        if (!ok) break;
        c.block_ops.push_back(new Exact<uint64_t>(k[0] * 3));
        ok = read_exact(f, c.block_ops.back()->p, k[0] * 24);
        c.blocks.push_back(rv_link_block{k[0] ? (const rv_op*)c.block_ops.back()->p : nullptr, k[0], k[1], k[2]});
    }
    if (ok) {
        c.block_of = new Exact<uint32_t>(h[1]), c.bindings = new Exact<uint32_t>(h[2]);
        c.head = new Exact<uint64_t>(h[5] * 3), c.tail = new Exact<uint64_t>(h[6] * 3);
        ok = read_exact(f, c.block_of->p, h[1] * 4) && read_exact(f, c.bindings->p, h[2] * 4) && read_exact(f, c.head->p, h[5] * 24) &&
             read_exact(f, c.tail->p, h[6] * 24);
    }
    fclose(f);
    if (!ok) return false;
    c.d.blocks = c.blocks.empty() ? nullptr : c.blocks.data(), c.d.n_blocks = h[0];
    c.d.block_of = h[1] ? c.block_of->p : nullptr, c.d.n_instances = h[1];
    c.d.bindings = h[2] ? c.bindings->p : nullptr, c.d.n_bindings = h[2];
    c.d.z64_base = h[3], c.d.gf2_base = h[4];
    c.d.head = h[5] ? (const rv_op*)c.head->p : nullptr, c.d.n_head = h[5];
    c.d.tail = h[6] ? (const rv_op*)c.tail->p : nullptr, c.d.n_tail = h[6];
    return true;
}

static uint64_t fnv(const uint8_t* p, size_t n) {
    uint64_t h = 0xCBF29CE484222325ull;
    for (size_t i = 0; i < n; i++) h = (h ^ p[i]) * 0x100000001B3ull;
    return h;
}

// ---- the plan, as link_plan_create builds it ----
struct BlockOff {
    const LkBlock* blk;
    uint64_t operator[](uint64_t i) const { return blk[i].off; }
};
struct Plan {
    Exact<uint64_t>* ops = nullptr;  // the blocks' records, head, tail
    Exact<LkBlock>* blk = nullptr;
    Exact<uint32_t>*ports = nullptr, *block_of = nullptr, *bindings = nullptr;
    Exact<uint64_t>*off = nullptr, *Z = nullptr, *G = nullptr, *B = nullptr;
    uint64_t n_inst = 0, n_head = 0, inst_ops = 0, head_at = 0, tail_at = 0;
    uint32_t zb = 0, gb = 0;
    rv_link_info info = {};
    ~Plan() {
        delete ops, delete blk, delete ports, delete block_of, delete bindings, delete off, delete Z, delete G, delete B;
    }
};

template <class T>
static void scan_excl(Exact<T>& a) {
    T run = 0;
    for (size_t i = 0; i < a.n; i++) {
        const T v = a[i];
        a[i] = run, run += v;
    }
}

// -> rv_link's code for the descriptor (RV_OK: the plan is made)
static int create(const rv_link_desc* d, Plan& P) {
    uint64_t block_ops = 0;
    if (const int rc = lk_check_args(d, &block_ops)) return rc;
    const uint64_t n_inst = d->n_instances, n_bind = d->n_bindings;
    P.ops = new Exact<uint64_t>((block_ops + d->n_head + d->n_tail) * 3);
    P.blk = new Exact<LkBlock>(d->n_blocks);
    P.ports = new Exact<uint32_t>(block_ops + 1);
    P.block_of = new Exact<uint32_t>(n_inst), P.bindings = new Exact<uint32_t>(n_bind);
    P.off = new Exact<uint64_t>(n_inst + 1), P.Z = new Exact<uint64_t>(n_inst + 1), P.G = new Exact<uint64_t>(n_inst + 1), P.B = new Exact<uint64_t>(n_inst + 1);
    uint64_t at = 0;
    for (uint64_t b = 0; b < d->n_blocks; b++) {
        const rv_link_block& k = d->blocks[b];
        (*P.blk)[b] = LkBlock{at, k.n_ops, k.z64_wires, k.gf2_wires};
        if (k.n_ops) memcpy(P.ops->p + at * 3, k.ops, k.n_ops * 24);
        at += k.n_ops;
    }
    if (d->n_head) memcpy(P.ops->p + at * 3, d->head, d->n_head * 24);
    if (d->n_tail) memcpy(P.ops->p + (at + d->n_head) * 3, d->tail, d->n_tail * 24);
    if (n_inst) memcpy(P.block_of->p, d->block_of, n_inst * 4);
    if (n_bind) memcpy(P.bindings->p, d->bindings, n_bind * 4);
    // k_link_judge: one thread per block record (and one more)
    uint64_t err_block = LK_NO_ERR, err_inst = LK_NO_ERR, err_bind = LK_NO_ERR;
    for (uint64_t r = 0; r <= block_ops; r++) {
        if (r == block_ops) {
            (*P.ports)[r] = 0;
            break;
        }
        const BlockOff offs{P.blk->p};
        const LkBlock& k = (*P.blk)[lk_last_le(offs, 0, d->n_blocks, r)];
        const uint64_t* w = P.ops->p + r * 3;
        const int code = lk_judge(w, k.z64_wires, k.gf2_wires);
        if (code) err_block = std::min(err_block, r << 8 | (uint64_t)code);
        (*P.ports)[r] = lk_is_input(w[0]) ? 1u : 0u;
    }
    scan_excl(*P.ports);
    // k_link_gather: one thread per instance (and one more)
    for (uint64_t i = 0; i <= n_inst; i++) {
        uint64_t v[4] = {0, 0, 0, 0};
        if (i < n_inst) {
            const uint32_t b = (*P.block_of)[i];
            if (b < d->n_blocks) {
                const LkBlock k = (*P.blk)[b];
                v[0] = k.n_ops, v[1] = k.z64_wires, v[2] = k.gf2_wires, v[3] = (*P.ports)[k.off + k.n_ops] - (*P.ports)[k.off];
            } else {
                err_inst = std::min(err_inst, i << 8 | (uint64_t)RV_E_ARG);
            }
        }
        (*P.off)[i] = v[0], (*P.Z)[i] = v[1], (*P.G)[i] = v[2], (*P.B)[i] = v[3];
    }
    scan_excl(*P.off), scan_excl(*P.Z), scan_excl(*P.G), scan_excl(*P.B);
    // the host's decisions
    if (err_block != LK_NO_ERR) return (int)(err_block & 0xFF);
    LkEnds ends;
    if (const int c = lk_judge_end(d->head, d->n_head, ends)) return c;
    if (const int c = lk_judge_end(d->tail, d->n_tail, ends)) return c;
    if (err_inst != LK_NO_ERR) return (int)(err_inst & 0xFF);
    if (n_bind != (*P.B)[n_inst]) return RV_E_ARG;
    if (const int c = lk_wire_counts(d, ends, (*P.Z)[n_inst], (*P.G)[n_inst], &P.info.z64_wires, &P.info.gf2_wires)) return c;
    // k_link_bind: one thread per binding
    uint64_t in[2] = {0, 0};
    for (uint64_t k = 0; k < n_bind; k++) {
        const uint64_t i = lk_last_le(P.B->p, 0, n_inst, k);
        const LkBlock b = (*P.blk)[(*P.block_of)[i]];
        const uint32_t* po = P.ports->p + b.off;
        const uint32_t port = (uint32_t)(k - (*P.B)[i]) + po[0];
        const uint64_t r = lk_last_le(po, 0, b.n_ops, port);
        const bool gf2 = lk_dom((*P.ops)[(b.off + r) * 3]) == RV_DOM_GF2;
        const uint32_t v = (*P.bindings)[k];
        if (v == RV_LINK_WITNESS) in[gf2 ? 0 : 1]++;
        else if ((uint64_t)v >= (gf2 ? P.info.gf2_wires : P.info.z64_wires)) err_bind = std::min(err_bind, k << 8 | (uint64_t)RV_E_WIRE_OOB);
    }
    if (err_bind != LK_NO_ERR) return (int)(err_bind & 0xFF);
    P.n_inst = n_inst, P.n_head = d->n_head, P.inst_ops = (*P.off)[n_inst], P.head_at = block_ops, P.tail_at = block_ops + d->n_head;
    P.zb = (uint32_t)d->z64_base, P.gb = (uint32_t)d->gf2_base;
    P.info.n_ops = d->n_head + P.inst_ops + d->n_tail, P.info.n_instances = n_inst;
    P.info.n_input_gf2 = ends.in_gf2 + in[0], P.info.n_input_z64 = ends.in_z64 + in[1];
    return RV_OK;
}

// k_link_emit: records [first, first + n) into out (n * 24 bytes; `addr` stands for its address: only addr mod 16 matters)
static void emit(const Plan& P, uint64_t first, uint64_t n, uint8_t* out, uintptr_t addr, uint64_t counts[2]) {
    const uint32_t TB = LINK_TILE;
    counts[0] = counts[1] = 0;
    for (uint64_t block = 0; block * TB < n; block++) {
        Exact<uint8_t> raw(LK_IMAGE);
        const uint64_t t0 = block * TB;
        const uint32_t mine = (uint32_t)std::min<uint64_t>(TB, n - t0);
        const uint32_t sh = (uint32_t)((addr + t0 * 24) & 15u);
        const uint64_t j0 = first + t0, jn = j0 + mine;
        uint64_t i0 = 0;
        if (jn > P.n_head && j0 < P.n_head + P.inst_ops) i0 = lk_last_le(P.off->p, 0, P.n_inst, j0 > P.n_head ? j0 - P.n_head : 0);
        for (uint32_t t = 0; t < mine; t++) {
            const uint64_t j = j0 + t;
            uint64_t o[3];
            if (j < P.n_head) {
                memcpy(o, P.ops->p + (P.head_at + j) * 3, 24);
            } else if (j >= P.n_head + P.inst_ops) {
                memcpy(o, P.ops->p + (P.tail_at + (j - P.n_head - P.inst_ops)) * 3, 24);
            } else {
                const uint64_t k = j - P.n_head;
                const uint64_t i = lk_gallop(P.off->p, i0, P.n_inst, k);
                const LkBlock b = (*P.blk)[(*P.block_of)[i]];
                const uint64_t r = b.off + (k - (*P.off)[i]);
                const uint64_t* w = P.ops->p + r * 3;
                uint32_t binding = 0;
                if (lk_is_input(w[0])) binding = (*P.bindings)[(*P.B)[i] + ((*P.ports)[r] - (*P.ports)[b.off])];
                lk_rewrite(w, P.zb + (uint32_t)(*P.Z)[i], P.gb + (uint32_t)(*P.G)[i], binding, o);
            }
            memcpy(raw.p + sh + t * 24, o, 24);
            if (lk_is_input(o[0])) counts[lk_dom(o[0]) == RV_DOM_GF2 ? 0 : 1]++;
        }
        const uint32_t span = sh + mine * 24;
        uint8_t* g0 = out + t0 * 24;  // the image's byte sh
        for (uint32_t t = 0; t < TB; t++)
            for (uint32_t c = t * 16; c < span; c += TB * 16) {
                const uint32_t kind = lk_chunk(c, sh, span);
                if (kind == 3) memcpy(g0 + c - sh, raw.p + c, 16);
                else if (kind == 1) memcpy(g0 + c - sh, raw.p + c, 8);
                else if (kind == 2) memcpy(g0 + (c + 8 - sh), raw.p + c + 8, 8);
            }
    }
}

// the range against rv_link's list, into an aligned buffer and into one that is 8 bytes off
static void check_range(const Plan& P, const uint64_t* want, uint64_t first, uint64_t n) {
    for (uintptr_t addr : {(uintptr_t)0, (uintptr_t)8}) {
        Exact<uint8_t> out(n * 24);
        uint64_t counts[2], in[2] = {0, 0};
        emit(P, first, n, out.p, addr, counts);
        EXPECT(n == 0 || memcmp(out.p, want + first * 3, n * 24) == 0);
        for (uint64_t j = first; j < first + n; j++)
            if (lk_is_input(want[j * 3])) in[lk_dom(want[j * 3]) == RV_DOM_GF2 ? 0 : 1]++;
        EXPECT(counts[0] == in[0] && counts[1] == in[1]);
    }
}

int main(int argc, char** argv) {
    bool ranges = false;
    for (int a = 1; a < argc; a++) {
        if (!strcmp(argv[a], "--ranges")) {
            ranges = true;
            continue;
        }
        const char* slash = strrchr(argv[a], '/');
        const std::string name = slash ? slash + 1 : argv[a];
        g_name = name.c_str();
        Case c;
        if (!load(argv[a], c)) {
            fprintf(stderr, "cannot read %s\n", argv[a]);
            return 2;
        }
        rv_op* linked = nullptr;
        rv_link_info info = {};
        const int code = rv_link(&c.d, &linked, &info);
        EXPECT((code == RV_OK) == (linked != nullptr));
        Plan P;
        const int model = create(&c.d, P);
        EXPECT(model == code);
        if (code == RV_OK && model == RV_OK) {
            EXPECT(memcmp(&P.info, &info, sizeof info) == 0);
            const uint64_t* want = (const uint64_t*)linked;
            check_range(P, want, 0, info.n_ops);
            uint64_t count = 0;
            if (ranges) {
                for (uint64_t first = 0; first <= info.n_ops; first++)
                    for (uint64_t n = 0; first + n <= info.n_ops; n++) check_range(P, want, first, n), count++;
            }
            printf("%s %d %llu %016llx\n", name.c_str(), code, (unsigned long long)info.n_ops, (unsigned long long)fnv((const uint8_t*)linked, info.n_ops * 24));
            if (ranges) printf("ranges %s %llu\n", name.c_str(), (unsigned long long)count);
        } else {
            printf("%s %d 0 0\n", name.c_str(), code);
        }
        free(linked);
    }
    printf("bad %d\n", g_bad);
    return g_bad ? 1 : 0;
}
