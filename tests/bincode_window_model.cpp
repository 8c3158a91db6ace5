// Stand-alone host program around the windowed program-file reader (rv_program_reader_*), built with -fsanitize=address,undefined by
// tests/test_bincode_window_host.py.  The state machine between the windows (bc_window_*: the carry rule, the offsets, what becomes
// final when), the record that straddles two windows (bc_enter) and the tile walk, map composition and decode are the functions of
// reverie_amd/csrc/bincode_dev.h the library runs; here a window's kernels are plain loops in the kernels' order.  Every window is a
// heap block of exactly its bytes, every tile of a window a heap block of exactly the bytes a workgroup may stage, and the carry put
// before a window's head a block of exactly those bytes: a read behind a window is a sanitizer report.  For every way of cutting,
// the records of all feeds, every feed's piece and the first nonzero code are compared with rv_program_from_bincode (program.cpp,
// linked in) on the whole file.
//
//   bincode_window_model FILE...                 every file cut into two windows: at every position (files up to EVERY_CUT_BYTES), or
//                                                at every position near its two ends and near the first tile boundary, around the
//                                                first scan block's end and at seeded random positions (longer files: every cut
//                                                costs a pass over the whole file, so a megabyte cut at every byte is out of reach)
//   bincode_window_model --fixed FILE...         ... and the files that follow fed 1 byte at a time and in windows of 31, 32, 33 bytes
//   bincode_window_model --mutations N FILE      ... and N seeded random byte mutations of the file that follows, at random cuts
//   bincode_window_model --resume FILE           a reader placed at file offsets 2^32 - 40 and 2^40 (rv_hook_program_reader_resume's
//                                                state), fed FILE's records: ordinals, info.bytes
// Prints "cuts K" per file, "fixed L", "mutations N", "resume 2", and "bad K" at the end (K mismatches).
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "bincode_dev.h"

using namespace rv;

constexpr size_t EVERY_CUT_BYTES = 13000;

struct HeapReader {
    const uint8_t* p;
    uint32_t u8(uint32_t o) const { return p[o]; }
    uint32_t u32(uint32_t o) const {
        uint32_t v;
        memcpy(&v, p + o, 4);
        return v;
    }
    uint64_t u64(uint32_t o) const {
        uint64_t v;
        memcpy(&v, p + o, 8);
        return v;
    }
};
struct Heap {  // exactly n bytes
    uint8_t* p;
    size_t n;
    Heap(const uint8_t* src, size_t n_) : p((uint8_t*)malloc(n_ ? n_ : 1)), n(n_) {
        if (n) memcpy(p, src, n);
    }
    ~Heap() { free(p); }
    Heap(const Heap&) = delete;
};
struct Tile : Heap {
    uint32_t avail;
    static size_t hi(size_t len, size_t t) { return std::min<size_t>(t * BINCODE_TILE_BYTES + BINCODE_TILE_BYTES + BC_MAX_RECORD - 1, len); }
    Tile(const uint8_t* data, size_t len, size_t t) : Heap(data + t * BINCODE_TILE_BYTES, hi(len, t) - t * BINCODE_TILE_BYTES), avail((uint32_t)n) {}
};

static void add_info(BcWindowResult& res, const uint64_t w[3], uint32_t dom) {
    uint64_t z, g;
    bc_wire_needs(w, z, g);
    res.info[BC_I_GF2 + dom]++;
    res.info[BC_I_Z64_WIRES] = std::max(res.info[BC_I_Z64_WIRES], z), res.info[BC_I_GF2_WIRES] = std::max(res.info[BC_I_GF2_WIRES], g);
    if (bc_is_input(w, RV_DOM_GF2)) res.info[BC_I_IN_GF2]++;
    if (bc_is_input(w, RV_DOM_Z64)) res.info[BC_I_IN_Z64]++;
}

// one window's kernels (bincode_dev.hip: k_bc_enter, walk, blocks, chase, resolve, decode) on data[0, len), len >= 1
static BcWindowResult window_model(const uint8_t* data, size_t len, const BcWindowLaunch& L, const uint8_t* carry, std::vector<rv_op>& out) {
    BcWindowResult res = {};
    res.err = res.stop = BC_NO_ERR;
    const uint64_t count = L.remaining;
    const size_t T = BINCODE_TILE_BYTES, B = BINCODE_SCAN_TILES, E = BC_ENTRIES;
    const size_t n_tiles = (len + T - 1) / T, n_blocks = (n_tiles + B - 1) / B;
    out.assign(len / BC_MIN_RECORD + 1, rv_op{});
    std::vector<uint8_t> seen(out.size(), 0);
    // enter
    BcChain c0{L.entry, 0, 0};
    if (L.carry_len) {
        const uint32_t c = L.carry_len;
        Tile t0(data, len, 0);
        const uint32_t m = std::min<uint32_t>(t0.avail, BC_MAX_RECORD - 1);
        std::vector<uint8_t> both(carry, carry + c);
        both.insert(both.end(), t0.p, t0.p + m);
        Heap buf(both.data(), both.size());
        const BcEnter e = bc_enter(BcBytes{buf.p}, c, c + m);
        res.straddle = e.straddle;
        if (e.straddle == 2) {
            c0 = BcChain{0, 1, 0};
            res.stop = 0;
            memcpy(res.tail, buf.p + c, m);
        } else {
            c0 = BcChain{e.entry, 0, 1};
            if (e.code) res.err = (uint64_t)e.code;
            else add_info(res, e.w, e.dom);
            if (count == 1) res.bytes_end = e.entry;
            memcpy(&out[0], e.w, sizeof(rv_op));
            seen[0]++;
        }
    }
    // walk, blocks
    std::vector<uint16_t> maps(n_tiles * E);
    for (size_t t = 0; t < n_tiles; t++) {
        Tile tile(data, len, t);
        for (uint32_t e = 0; e < E; e++) maps[t * E + e] = (uint16_t)bc_walk_tile(HeapReader{tile.p}, tile.avail, e, nullptr);
    }
    std::vector<uint64_t> bmaps(n_blocks * E);
    for (size_t b = 0; b < n_blocks; b++)
        for (uint32_t e = 0; e < E; e++) {
            BcChain c{e, 0, 0};
            for (size_t t = b * B; t < std::min(n_tiles, (b + 1) * B) && !c.stopped; t++) bc_chain_step(c, maps[t * E + c.entry]);
            bmaps[b * E + e] = bc_block_entry(c);
        }
    // chase, resolve
    std::vector<uint64_t> block_in(n_blocks), tile_in(n_tiles);
    BcChain c{0, 0, 0};
    bc_chain_block(c, bc_block_entry(c0));
    for (size_t b = 0; b < n_blocks; b++) {
        block_in[b] = bc_block_entry(c);
        if (!c.stopped) bc_chain_block(c, bmaps[b * E + c.entry]);
    }
    res.found = c.records;
    for (size_t b = 0; b < n_blocks; b++) {
        BcChain k{0, 0, 0};
        bc_chain_block(k, block_in[b]);
        for (size_t t = b * B; t < std::min(n_tiles, (b + 1) * B); t++) {
            tile_in[t] = bc_block_entry(k);
            if (!k.stopped) bc_chain_step(k, maps[t * E + k.entry]);
        }
    }
    // decode
    for (size_t t = 0; t < n_tiles; t++) {
        const uint64_t first = tile_in[t] & 0xFFFFFFFFull;
        if ((uint32_t)(tile_in[t] >> 32) == BC_STOP || first >= count) continue;
        Tile tile(data, len, t);
        const HeapReader r{tile.p};
        uint16_t starts[BC_TILE_RECORDS];
        uint32_t end;
        const uint32_t m = bc_walk_tile(r, tile.avail, (uint32_t)(tile_in[t] >> 32), starts, &end);
        if ((m & 63u) == BC_STOP) {
            res.stop = t * T + end;
            if (t * T + tile.avail == len && tile.avail - end < BC_MAX_RECORD)
                for (uint32_t k = end; k < tile.avail; k++) res.tail[k - end] = (uint8_t)r.u8(k);
        }
        const uint32_t n = (uint32_t)std::min<uint64_t>(m >> 6, count - first);
        for (uint32_t i = 0; i < n; i++) {
            uint32_t dom = 0, opc = 0;
            const uint32_t rec_len = bc_peek(r, starts[i], tile.avail, dom, opc);
            uint64_t w[3];
            const int code = bc_decode(r, starts[i], dom, opc, w);
            if (code) res.err = std::min(res.err, (first + i) << 8 | (uint64_t)code);
            else add_info(res, w, dom);
            if (first + i == count - 1) res.bytes_end = t * T + starts[i] + rec_len;
            memcpy(&out.at(first + i), w, sizeof(rv_op));  // (len / 16 + 1 records are room enough: .at)
            seen.at(first + i)++;
        }
    }
    const uint64_t deliver = std::min<uint64_t>(res.found, count);
    for (size_t i = 0; i < seen.size(); i++)
        if (seen[i] != (i < deliver ? 1 : 0)) res.err = 0xFF;  // (every delivered record decoded exactly once, none behind them)
    return res;
}

// rv_program_reader_feed with the model for the kernels; the window is an exact heap block
static int feed_model(BcWindowState& s, const uint8_t* bytes, size_t len, std::vector<rv_op>& out, rv_program_piece* piece) {
    out.clear();
    if (s.code || len > s.file_len - s.file_off) return RV_E_ARG;
    Heap win(bytes, len);
    uint32_t head_taken = 0;
    if (!s.have_count) {
        head_taken = bc_window_head_need(s, len);
        if (int code = bc_window_head(s, win.p, head_taken, len)) return code;
        if (!s.have_count) return *piece = rv_program_piece{}, 0;
    }
    if (s.done || !len) return bc_window_skip(s, len, piece), 0;
    const BcWindowResult res = window_model(win.p, len, bc_window_launch(s, head_taken), s.carry, out);
    const int code = bc_window_done(s, len, res, piece);
    out.resize(code ? 0 : (size_t)piece->n_ops);
    return code;
}

static uint32_t op_len(const rv_op& g) {
    uint64_t w[3];
    memcpy(w, &g, sizeof g);
    return bc_op_len(w);
}
static rv_program_info info_of(const rv_op* ops, size_t n) {
    rv_program_info in = {};
    in.n_ops = n, in.bytes = 8;
    for (size_t i = 0; i < n; i++) {
        uint64_t w[3], z, g;
        memcpy(w, &ops[i], sizeof(rv_op));
        bc_wire_needs(w, z, g);
        in.bytes += op_len(ops[i]);
        (ops[i].domain == 0 ? in.n_gf2 : ops[i].domain == 1 ? in.n_z64 : ops[i].domain == 2 ? in.n_b2a : in.n_sizehint)++;
        in.z64_wires = std::max(in.z64_wires, z), in.gf2_wires = std::max(in.gf2_wires, g);
    }
    return in;
}

struct Whole {  // the host reader's answer for a file
    int rc;
    rv_op* ops = nullptr;
    size_t n = 0;
    std::vector<uint64_t> ends;  // file offset behind record i
    Whole(const uint8_t* bytes, size_t len) {
        Heap copy(bytes, len);
        rc = rv_program_from_bincode(copy.p, len, &ops, &n);
        uint64_t at = 8;
        for (size_t i = 0; i < n; i++) ends.push_back(at += op_len(ops[i]));
    }
    ~Whole() { free(ops); }
};

// 1 if the windows (their lengths; they need not cover the file) disagree with the host reader
static int compare(const char* what, const uint8_t* bytes, size_t len, const Whole& W, const std::vector<size_t>& windows) {
    BcWindowState s;
    bc_window_begin(s, len);
    std::vector<rv_op> all, out;
    int code = 0;
    size_t at = 0, k = 0;
    for (; k < windows.size() && !code; k++) {
        rv_program_piece piece = {};
        code = feed_model(s, bytes + at, windows[k], out, &piece);
        at += windows[k];
        if (code) break;
        // the defined number: the records not yet delivered that end inside the bytes fed so far
        size_t want = 0;
        if (W.rc == RV_OK) want = (size_t)(std::upper_bound(W.ends.begin(), W.ends.end(), (uint64_t)at) - W.ends.begin()) - all.size();
        if (W.rc == RV_OK && (piece.n_ops != want || piece.first_op != all.size())) {
            printf("MISMATCH %s window %zu (%zu bytes, ends at %zu): n_ops %llu first_op %llu, want %zu %zu\n", what, k, windows[k], at,
                   (unsigned long long)piece.n_ops, (unsigned long long)piece.first_op, want, all.size());
            return 1;
        }
        uint64_t in_gf2 = 0, in_z64 = 0;
        for (const rv_op& g : out) in_gf2 += g.domain == 0 && g.opcode == 0, in_z64 += g.domain == 1 && g.opcode == 0;
        if (piece.n_input_gf2 != in_gf2 || piece.n_input_z64 != in_z64) return printf("MISMATCH %s window %zu: input counts\n", what, k), 1;
        all.insert(all.end(), out.begin(), out.end());
    }
    rv_program_info info = {};
    if (!code && at == len) code = bc_window_finish(s, &info) == RV_OK ? 0 : RV_E_BAD_OP + 100;  // (a whole file without a code must finish)
    int bad = at == len ? code != W.rc : (code != 0 && code != W.rc);
    if (!bad && W.rc == RV_OK && at == len) {
        const rv_program_info want = info_of(W.ops, W.n);
        bad = all.size() != W.n || (W.n && memcmp(all.data(), W.ops, W.n * sizeof(rv_op))) || memcmp(&want, &info, sizeof want);
    }
    // after a code the reader takes nothing more
    if (code && code < 100 && !bad) {
        rv_program_piece piece;
        bad = feed_model(s, bytes, 0, out, &piece) != RV_E_ARG || bc_window_finish(s, &info) != RV_E_ARG;
    }
    if (bad) {
        printf("MISMATCH %s len %zu windows", what, len);
        for (size_t w : windows) printf(" %zu", w);
        printf(": host %d / %zu, model %d / %zu\n", W.rc, W.n, code, all.size());
    }
    return bad;
}

static std::vector<size_t> fixed_windows(size_t len, size_t w) {
    std::vector<size_t> v;
    for (size_t at = 0; at < len; at += w) v.push_back(std::min(w, len - at));
    if (v.empty()) v.push_back(0);
    return v;
}

static uint64_t g_seed = 0x9E3779B97F4A7C15ull;
static uint64_t next_random() {  // splitmix64
    uint64_t z = (g_seed += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

// a reader placed at file offset off with `first` records behind it, fed body (whole records) in windows of 100 bytes
static int resume_run(const uint8_t* body, size_t n_body, uint64_t off, uint64_t first, const Whole& W) {
    BcWindowState s;
    bc_window_begin(s, off + n_body);
    bc_window_resume(s, off, first);
    std::vector<rv_op> all, out;
    size_t at = 0;
    for (size_t w : fixed_windows(n_body, 100)) {
        rv_program_piece piece = {};
        if (feed_model(s, body + at, w, out, &piece)) return 1;
        if (piece.first_op != first + all.size()) return 1;
        at += w;
        all.insert(all.end(), out.begin(), out.end());
    }
    rv_program_info info = {};
    if (bc_window_finish(s, &info) != RV_OK) return 1;
    if (info.bytes != off + n_body || info.n_ops != first + W.n || s.file_off != off + n_body) return 1;
    return all.size() != W.n || memcmp(all.data(), W.ops, W.n * sizeof(rv_op)) != 0;
}

int main(int argc, char** argv) {
    static_assert(sizeof(rv_program_info) == 64 && sizeof(rv_op) == 24 && sizeof(rv_program_piece) == 32, "layouts of the header");
    bool fixed = false, resume = false;
    long mutations = 0;
    int bad = 0;
    for (int a = 1; a < argc; a++) {
        if (!strcmp(argv[a], "--fixed")) {
            fixed = true;
            continue;
        }
        if (!strcmp(argv[a], "--resume")) {
            resume = true;
            continue;
        }
        if (!strcmp(argv[a], "--mutations") && a + 1 < argc) {
            mutations = atol(argv[++a]);
            continue;
        }
        FILE* f = fopen(argv[a], "rb");
        if (!f) return 2;
        std::vector<uint8_t> d;
        uint8_t buf[4096];
        for (size_t n; (n = fread(buf, 1, sizeof buf, f)) > 0;) d.insert(d.end(), buf, buf + n);
        fclose(f);
        const char* name = strrchr(argv[a], '/') ? strrchr(argv[a], '/') + 1 : argv[a];
        const Whole W(d.data(), d.size());
        if (resume) {
            if (W.rc != RV_OK || d.size() < 8) return 2;
            bad += resume_run(d.data() + 8, (size_t)W.ends.back() - 8, (1ull << 32) - 40, (1ull << 32) / 16, W);
            bad += resume_run(d.data() + 8, (size_t)W.ends.back() - 8, 1ull << 40, (1ull << 40) / 16 + 3, W);
            printf("resume 2\n");
            resume = false;
            continue;
        }
        // two windows
        std::vector<size_t> cuts;
        const size_t len = d.size(), T = BINCODE_TILE_BYTES;
        if (len <= EVERY_CUT_BYTES) {
            for (size_t c = 0; c <= len; c++) cuts.push_back(c);
        } else {
            const size_t reach = len <= (64u << 10) ? 40 : 5, BT = T * BINCODE_SCAN_TILES;
            for (size_t c = 0; c <= reach; c++) cuts.push_back(c), cuts.push_back(len - c);
            for (size_t c = T - reach; c <= T + reach; c++) cuts.push_back(c);
            if (len > BT + 1) cuts.push_back(BT - 1), cuts.push_back(BT), cuts.push_back(BT + 1);
            for (size_t k = 0; k < reach / 2; k++) cuts.push_back((size_t)(next_random() % (len + 1)));
        }
        for (size_t c : cuts) bad += compare(name, d.data(), len, W, {c, len - c});
        printf("cuts %zu\n", cuts.size());
        if (fixed) {
            for (size_t w : {(size_t)1, (size_t)31, (size_t)32, (size_t)33}) bad += compare(name, d.data(), len, W, fixed_windows(len, w));
            printf("fixed %zu\n", len);
        }
        if (mutations) {
            for (long m = 0; m < mutations; m++) {
                std::vector<uint8_t> x = d;
                for (int k = 1 + (int)(next_random() % 3); k > 0 && !x.empty(); k--) {
                    const size_t at = next_random() % x.size();
                    const uint64_t v = next_random();
                    x[at] = (v & 1) ? (uint8_t)(v >> 8) : (uint8_t)((v >> 8) % 11);
                }
                if (next_random() % 4 == 0) x.resize(next_random() % (x.size() + 1));  // a quarter of them cut short as well
                const Whole Wx(x.data(), x.size());
                // one to four cuts anywhere; one mutation in four in small windows around a mutated spot's size
                std::vector<size_t> at_cuts;
                for (int k = 1 + (int)(next_random() % 4); k > 0; k--) at_cuts.push_back((size_t)(next_random() % (x.size() + 1)));
                std::sort(at_cuts.begin(), at_cuts.end());
                std::vector<size_t> windows;
                size_t prev = 0;
                for (size_t c : at_cuts) windows.push_back(c - prev), prev = c;
                windows.push_back(x.size() - prev);
                bad += compare(name, x.data(), x.size(), Wx, windows);
            }
            printf("mutations %ld\n", mutations);
            mutations = 0;
        }
    }
    printf("bad %d\n", bad);
    return bad ? 1 : 0;
}
