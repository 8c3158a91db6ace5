// Stand-alone host program around the device bincode reader's functions (reverie_amd/csrc/bincode_dev.h), built with
// -fsanitize=address,undefined by tests/test_bincode_device_host.py.  The tile walk, the map composition and the record decode the
// kernels of bincode_dev.hip run are these same functions; here they run as plain loops in the kernels' order (walk every tile from
// every entry, compose the maps by blocks, chase the block maps, resolve, decode), and every tile is read from a heap block of
// exactly the bytes a workgroup may stage -- the tile and the 31 bytes behind it, clipped to the file's length -- so a read past
// them is a sanitizer report.  The answer (code, count, records, info) is compared with rv_program_from_bincode (program.cpp, linked
// in) on the same bytes: the check of the error rule that needs no GPU.
//
//   bincode_walk_asan FILE...                         every file whole
//   bincode_walk_asan --prefixes FILE...              ... and every prefix of the files that follow
//   bincode_walk_asan --mutations N FILE              ... and N seeded random byte mutations of the file that follows
// Prints one line per whole file (name, length, code, count), "prefixes L", "mutations N", and "bad K" at the end (K mismatches).
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "bincode_dev.h"

using namespace rv;

// a tile's bytes: a heap block of exactly `avail` bytes
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
struct Tile {
    uint8_t* block;
    uint32_t avail;
    Tile(const uint8_t* data, size_t len, size_t t) {
        const size_t lo = t * BINCODE_TILE_BYTES, hi = std::min<size_t>(lo + BINCODE_TILE_BYTES + BC_MAX_RECORD - 1, len);
        avail = (uint32_t)(hi - lo);
        block = (uint8_t*)malloc(avail ? avail : 1);
        memcpy(block, data + lo, avail);
    }
    ~Tile() { free(block); }
    Tile(const Tile&) = delete;
};

struct Answer {
    int code = 0;
    std::vector<rv_op> ops;
    rv_program_info info = {};
};

// rv_program_from_bincode_device's pipeline on the host
static Answer model(const uint8_t* data, size_t len) {
    Answer A;
    if (len < BC_HEADER_BYTES) return A.code = RV_E_BAD_OP, A;
    uint64_t count = 0;
    for (uint32_t k = 0; k < BC_HEADER_BYTES; k++) count |= (uint64_t)data[k] << (8 * k);
    if (count > (len - BC_HEADER_BYTES) / BC_MIN_RECORD) return A.code = RV_E_BAD_OP, A;
    A.info.bytes = BC_HEADER_BYTES;
    if (!count) return A;
    const size_t T = BINCODE_TILE_BYTES, B = BINCODE_SCAN_TILES, E = BC_ENTRIES;
    const size_t n_tiles = (len + T - 1) / T, n_blocks = (n_tiles + B - 1) / B;
    // 1. walk
    std::vector<uint16_t> maps(n_tiles * E);
    for (size_t t = 0; t < n_tiles; t++) {
        Tile tile(data, len, t);
        for (uint32_t e = 0; e < E; e++) maps[t * E + e] = (uint16_t)bc_walk_tile(HeapReader{tile.block}, tile.avail, e, nullptr);
    }
    // 2. blocks
    std::vector<uint64_t> bmaps(n_blocks * E);
    for (size_t b = 0; b < n_blocks; b++)
        for (uint32_t e = 0; e < E; e++) {
            BcChain c{e, 0, 0};
            for (size_t t = b * B; t < std::min(n_tiles, (b + 1) * B) && !c.stopped; t++) bc_chain_step(c, maps[t * E + c.entry]);
            bmaps[b * E + e] = bc_block_entry(c);
        }
    // 3. chase
    uint64_t err = ~0ull;
    std::vector<uint64_t> block_in(n_blocks);
    BcChain c{BC_HEADER_BYTES, 0, 0};
    for (size_t b = 0; b < n_blocks; b++) {
        block_in[b] = bc_block_entry(c);
        if (!c.stopped) bc_chain_block(c, bmaps[b * E + c.entry]);
    }
    if (c.records < count) err = c.records << 8 | (uint64_t)RV_E_BAD_OP;
    // 4. resolve
    std::vector<uint64_t> tile_in(n_tiles);
    for (size_t b = 0; b < n_blocks; b++) {
        BcChain k{0, 0, 0};
        bc_chain_block(k, block_in[b]);
        for (size_t t = b * B; t < std::min(n_tiles, (b + 1) * B); t++) {
            tile_in[t] = bc_block_entry(k);
            if (!k.stopped) bc_chain_step(k, maps[t * E + k.entry]);
        }
    }
    // 5. decode
    A.ops.assign((size_t)count, rv_op{});
    std::vector<uint8_t> seen((size_t)count, 0);
    for (size_t t = 0; t < n_tiles; t++) {
        const uint64_t first = tile_in[t] & 0xFFFFFFFFull;
        if ((uint32_t)(tile_in[t] >> 32) == BC_STOP || first >= count) continue;
        Tile tile(data, len, t);
        const HeapReader r{tile.block};
        uint16_t starts[BC_TILE_RECORDS];
        const uint32_t found = bc_walk_tile(r, tile.avail, (uint32_t)(tile_in[t] >> 32), starts) >> 6;
        const uint32_t n = (uint32_t)std::min<uint64_t>(found, count - first);
        for (uint32_t i = 0; i < n; i++) {
            uint32_t dom = 0, opc = 0;
            const uint32_t rec_len = bc_peek(r, starts[i], tile.avail, dom, opc);
            uint64_t w[3];
            const int code = bc_decode(r, starts[i], dom, opc, w);
            if (code) err = std::min(err, (first + i) << 8 | (uint64_t)code);
            else {
                uint64_t z, g;
                bc_wire_needs(w, z, g);
                (dom == 0 ? A.info.n_gf2 : dom == 1 ? A.info.n_z64 : dom == 2 ? A.info.n_b2a : A.info.n_sizehint)++;
                A.info.z64_wires = std::max(A.info.z64_wires, z), A.info.gf2_wires = std::max(A.info.gf2_wires, g);
            }
            if (first + i == count - 1) A.info.bytes = t * T + starts[i] + rec_len;
            memcpy(&A.ops[first + i], w, sizeof(rv_op));
            seen[first + i]++;
        }
    }
    if (err != ~0ull) {
        A.code = (int)(err & 0xFF);
        A.ops.clear();
        A.info = {};
        return A;
    }
    for (uint8_t s : seen)
        if (s != 1) A.code = -1;  // (every record decoded exactly once)
    A.info.n_ops = count;
    return A;
}

// an independent reading of rv_program_info from the host reader's records
static rv_program_info info_of(const rv_op* ops, size_t n) {
    rv_program_info in = {};
    in.n_ops = n, in.bytes = 8;
    for (size_t i = 0; i < n; i++) {
        const rv_op& g = ops[i];
        uint64_t z = 0, f = 0;
        if (g.domain == RV_DOM_B2A) in.n_b2a++, z = (uint64_t)g.dst + 1, f = (uint64_t)g.a + 64, in.bytes += 20;
        else if (g.domain == RV_DOM_SIZEHINT) in.n_sizehint++, z = g.a, f = g.b, in.bytes += 20;
        else {
            const int tb = g.domain == RV_DOM_GF2 ? 1 : 8;
            uint64_t hi = 0;
            const bool three = g.opcode == RV_OP_ADD || g.opcode == RV_OP_SUB || g.opcode == RV_OP_MUL;
            const bool cst = g.opcode == RV_OP_ADDCONST || g.opcode == RV_OP_SUBCONST || g.opcode == RV_OP_MULCONST;
            if (g.opcode != RV_OP_ASSERTZERO) hi = std::max<uint64_t>(hi, (uint64_t)g.dst + 1);
            if (three || cst || g.opcode == RV_OP_ASSERTZERO) hi = std::max<uint64_t>(hi, (uint64_t)g.a + 1);
            if (three) hi = std::max<uint64_t>(hi, (uint64_t)g.b + 1);
            in.bytes += 8 + (three ? 24 : cst ? 16 + tb : g.opcode == RV_OP_CONST ? 8 + tb : 8);
            (g.domain == RV_DOM_GF2 ? in.n_gf2 : in.n_z64)++;
            (g.domain == RV_DOM_GF2 ? f : z) = hi;
        }
        in.z64_wires = std::max(in.z64_wires, z), in.gf2_wires = std::max(in.gf2_wires, f);
    }
    return in;
}

// 1 if the model and the host reader disagree on bytes[0, len) (an exact-size heap copy for the host reader too)
static int compare(const char* what, const uint8_t* bytes, size_t len, bool print) {
    uint8_t* copy = (uint8_t*)malloc(len ? len : 1);
    if (len) memcpy(copy, bytes, len);
    rv_op* ops = nullptr;
    size_t n = 0;
    const int rc = rv_program_from_bincode(copy, len, &ops, &n);
    const Answer A = model(copy, len);
    int bad = A.code != rc;
    if (!bad && rc == RV_OK) {
        bad = A.ops.size() != n || (n && memcmp(A.ops.data(), ops, n * sizeof(rv_op)));
        const rv_program_info want = info_of(ops, n);
        bad |= memcmp(&want, &A.info, sizeof want) != 0;
    }
    if (print) printf("%s %zu %d %zu\n", what, len, rc, n);
    if (bad) printf("MISMATCH %s len %zu: host %d / %zu, model %d / %zu\n", what, len, rc, n, A.code, A.ops.size());
    free(ops);
    free(copy);
    return bad;
}

int main(int argc, char** argv) {
    static_assert(sizeof(rv_program_info) == 64 && sizeof(rv_op) == 24, "layouts of the header");
    bool prefixes = false;
    long mutations = 0;
    int bad = 0;
    for (int a = 1; a < argc; a++) {
        if (!strcmp(argv[a], "--prefixes")) {
            prefixes = true;
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
        bad += compare(name, d.data(), d.size(), true);
        if (prefixes) {
            for (size_t n = 0; n < d.size(); n++) bad += compare(name, d.data(), n, false);
            printf("prefixes %zu\n", d.size());
        }
        if (mutations) {
            uint64_t s = 0x9E3779B97F4A7C15ull;
            auto next = [&s]() {  // splitmix64
                uint64_t z = (s += 0x9E3779B97F4A7C15ull);
                z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
                z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
                return z ^ (z >> 31);
            };
            for (long m = 0; m < mutations; m++) {
                std::vector<uint8_t> x = d;
                // one to three bytes: any value, or one that lands on the rules' edges (a tag of 0 .. 10, a fifth wire byte of 1, a bool of 2)
                for (int k = 1 + (int)(next() % 3); k > 0 && !x.empty(); k--) {
                    const size_t at = next() % x.size();
                    const uint64_t v = next();
                    x[at] = (v & 1) ? (uint8_t)(v >> 8) : (uint8_t)((v >> 8) % 11);
                }
                const size_t cut = (next() % 4) ? x.size() : next() % (x.size() + 1);  // a quarter of them cut short as well
                bad += compare(name, x.data(), cut, false);
            }
            printf("mutations %ld\n", mutations);
            mutations = 0;
        }
    }
    printf("bad %d\n", bad);
    return bad ? 1 : 0;
}
