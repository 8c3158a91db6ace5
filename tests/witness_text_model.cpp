// The witness-text kernels' order of work on the CPU (test_witness_text_host.py builds this with -fsanitize=address,undefined): the
// lane, tile and writer rules of reverie_amd/csrc/witness_text.h -- what the kernels of witness_dev.hip run -- as plain loops, tile
// by tile, with every buffer a heap block of exactly its bytes, so that a load or a store one byte outside is caught.
//
//   witness_text_model FILE... [--cuts FILE...]
//
// For every FILE (a text): the two-pass parse (count, scan, scatter through the tile image with its 16-byte chunks) at every source
// alignment 0..15, with the destination alignment stepping along, against a byte loop; the marks rule at the tile edges; the writer,
// lane by lane, for the line lengths {0, 1, 7, 16, 64, n, n + 1} and every destination alignment, against a byte loop, and back
// through the parser.  Behind --cuts: also every two-way cut of the text, each part in a heap block of its own, and a mark at every
// position.  Prints "NAME count fnv(bits) fnv(text at line length 0) ..." per file, "checks N" and "bad N".
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

#include "witness_text.h"

using namespace rv;

static uint64_t g_checks = 0, g_bad = 0;
static void expect(bool ok, const char* what, const std::string& name) {
    g_checks++;
    if (!ok) {
        g_bad++;
        fprintf(stderr, "MISMATCH %s: %s\n", name.c_str(), what);
    }
}

// a heap block of exactly n bytes (n == 0: a block of one byte that nothing may touch is still "exactly": index 0 is never used)
struct Block {
    uint8_t* p;
    size_t n;
    explicit Block(size_t n_, int fill = 0xEE) : p((uint8_t*)malloc(n_ ? n_ : 1)), n(n_) { memset(p, fill, n_ ? n_ : 1); }
    Block(const Block&) = delete;
    ~Block() { free(p); }
};

static uint64_t fnv(const uint8_t* d, size_t n) {
    uint64_t h = 0xCBF29CE484222325ull;
    for (size_t i = 0; i < n; i++) h = (h ^ d[i]) * 0x100000001B3ull;
    return h;
}

static bool same(const uint8_t* p, const std::vector<uint8_t>& v) { return v.empty() || !memcmp(p, v.data(), v.size()); }

static std::vector<uint8_t> byte_loop(const uint8_t* t, size_t len) {
    std::vector<uint8_t> out;
    for (size_t i = 0; i < len; i++)
        if (t[i] == '0' || t[i] == '1') out.push_back((uint8_t)(t[i] - '0'));
    return out;
}

// the lane whose 16 bytes begin at text index `at` (it may begin before the text and end behind it), as the kernels load it
static void lane_load(const uint8_t* text, size_t len, int64_t at, uint32_t w[4]) {
    if (at >= 0 && (uint64_t)at + WT_LANE_BYTES <= len) {
        memcpy(w, text + at, WT_LANE_BYTES);  // the 16-byte load
    } else if (at + (int64_t)WT_LANE_BYTES > 0 && at < (int64_t)len) {
        // (the pointer is formed from an integer, as the kernel's: only the bytes inside [text, text + len) are read)
        const uint8_t* c = (const uint8_t*)((uintptr_t)text + (uintptr_t)at);
        wt_lane_bytes(c, text, text + len, w);
    } else {
        w[0] = w[1] = w[2] = w[3] = 0;
    }
}

struct Tiles {
    std::vector<uint32_t> offs;  // exclusive prefix of the tile counts
    uint32_t total = 0;
};

// the count pass and the scan: the text's first byte has address `shift` modulo 16
static Tiles count_pass(const uint8_t* text, size_t len, uint32_t shift) {
    Tiles T;
    const size_t n_tiles = len ? (shift + len + WT_TILE_BYTES - 1) / WT_TILE_BYTES : 0;
    for (size_t t = 0; t < n_tiles; t++) {
        uint32_t n = 0;
        for (uint32_t l = 0; l < WT_TILE_BYTES / WT_LANE_BYTES; l++) {
            uint32_t w[4];
            lane_load(text, len, (int64_t)(t * WT_TILE_BYTES + l * WT_LANE_BYTES) - shift, w);
            n += wt_lane_count(w);
        }
        T.offs.push_back(T.total);
        T.total += n;
    }
    return T;
}

// the scatter pass into out (a block of exactly T.total bytes whose first byte has address `dshift` modulo 16)
static void scatter_pass(const uint8_t* text, size_t len, uint32_t shift, const Tiles& T, uint8_t* out, uint32_t dshift) {
    for (size_t t = 0; t < T.offs.size(); t++) {
        Block image(16 + WT_TILE_BYTES + 16);
        const uint64_t g0 = T.offs[t];
        const uint32_t sh = (uint32_t)((dshift + g0) & 15u);
        uint32_t before = 0;
        for (uint32_t l = 0; l < WT_TILE_BYTES / WT_LANE_BYTES; l++) {
            uint32_t w[4];
            lane_load(text, len, (int64_t)(t * WT_TILE_BYTES + l * WT_LANE_BYTES) - shift, w);
            const uint32_t mask = wt_keep_mask(w);
            wt_lane_values(w, mask, image.p + sh + before);
            before += (uint32_t)__builtin_popcount(mask);
        }
        const uint32_t span = sh + before;
        for (uint32_t at = 0; at < span; at += 16) {
            if (wt_chunk_whole(at, sh, span)) {
                memcpy(out + (g0 + at - sh), image.p + at, 16);  // the 16-byte store
            } else {
                for (uint32_t k = 0; k < 16; k++)
                    if (at + k >= sh && at + k < span) out[g0 + at + k - sh] = image.p[at + k];
            }
        }
    }
}

// the marks rule: the bits of text[0, p)
static uint64_t mark_rule(const uint8_t* text, size_t len, uint32_t shift, const Tiles& T, uint64_t p) {
    const uint64_t q = shift + p;
    const size_t tile = (size_t)(q / WT_TILE_BYTES);
    if (tile >= T.offs.size()) return T.total;
    uint32_t n = 0;
    for (uint32_t l = 0; l < WT_TILE_BYTES / WT_LANE_BYTES; l++) {
        uint32_t w[4];
        lane_load(text, (size_t)p, (int64_t)(tile * WT_TILE_BYTES + l * WT_LANE_BYTES) - shift, w);
        n += wt_lane_count(w);
    }
    (void)len;
    return (uint64_t)T.offs[tile] + n;
}

static std::vector<uint8_t> parse_model(const uint8_t* text, size_t len, uint32_t shift, uint32_t dshift) {
    const Tiles T = count_pass(text, len, shift);
    Block out(T.total);
    scatter_pass(text, len, shift, T, out.p, dshift);
    return std::vector<uint8_t>(out.p, out.p + T.total);
}

// the writer, lane by lane, into a block of exactly the text's bytes whose first byte has address `shift` modulo 16
static std::vector<uint8_t> write_model(const uint8_t* bits, size_t n, uint64_t line_bits, uint32_t shift, bool* bad) {
    const uint64_t len = wt_text_len(n, line_bits), L = wt_line(n, line_bits);
    Block out((size_t)len);
    *bad = false;
    for (uint64_t a = 0; a < shift + len; a += 16) {
        uint64_t j0, j1;
        wt_lane_range(a, shift, len, &j0, &j1);
        if (j0 >= j1) continue;
        if (j1 - j0 == 16) {
            uint8_t v[16];
            *bad |= wt_write_range(j0, j1, L, n, bits, v);
            memcpy(out.p + j0, v, 16);  // the 16-byte store
        } else {
            *bad |= wt_write_range(j0, j1, L, n, bits, out.p + j0);
        }
    }
    return std::vector<uint8_t>(out.p, out.p + len);
}

static std::vector<uint8_t> write_loop(const uint8_t* bits, size_t n, uint64_t line_bits) {
    std::vector<uint8_t> out;
    for (size_t i = 0; i < n; i++) {
        out.push_back((uint8_t)('0' + bits[i]));
        if ((line_bits && (i + 1) % line_bits == 0) || i == n - 1) out.push_back('\n');
    }
    return out;
}

static void run_file(const char* path, bool cuts) {
    FILE* f = fopen(path, "rb");
    if (!f) {
        fprintf(stderr, "cannot open %s\n", path);
        exit(2);
    }
    std::vector<uint8_t> data;
    uint8_t buf[4096];
    for (size_t got; (got = fread(buf, 1, sizeof buf, f)) > 0;) data.insert(data.end(), buf, buf + got);
    fclose(f);
    std::string name = path;
    name = name.substr(name.find_last_of('/') + 1);
    const size_t len = data.size();
    Block text(len);
    if (len) memcpy(text.p, data.data(), len);
    const std::vector<uint8_t> want = byte_loop(text.p, len);

    // the parse at every source alignment; the destination alignment steps along, so that all 16 are met
    for (uint32_t shift = 0; shift < 16; shift++) {
        const std::vector<uint8_t> got = parse_model(text.p, len, shift, (shift * 7 + 3) & 15u);
        expect(got == want, "parse", name);
        const Tiles T = count_pass(text.p, len, shift);
        expect(T.total == want.size(), "count", name);
        // marks at 0, at len and one byte around every tile edge of this alignment
        std::vector<uint64_t> marks = {0, len};
        for (size_t t = 1; t <= T.offs.size(); t++)
            for (int d = -1; d <= 1; d++) {
                const int64_t p = (int64_t)(t * WT_TILE_BYTES) - shift + d;
                if (p >= 0 && (uint64_t)p <= len) marks.push_back((uint64_t)p);
            }
        if (cuts)
            for (uint64_t p = 0; p <= len; p++) marks.push_back(p);
        for (uint64_t p : marks) expect(mark_rule(text.p, len, shift, T, p) == byte_loop(text.p, (size_t)p).size(), "mark", name);
    }
    // the host functions say the same
    {
        size_t n = 0;
        expect(rv_witness_parse((const char*)text.p, len, nullptr, 0, &n) == RV_OK && n == want.size(), "host count", name);
        Block bits(want.size());
        expect(rv_witness_parse((const char*)text.p, len, bits.p, want.size(), &n) == RV_OK && same(bits.p, want), "host parse", name);
        if (!want.empty()) {
            Block small(want.size() - 1, 0x5A);
            bool kept = rv_witness_parse((const char*)text.p, len, small.p, want.size() - 1, &n) == RV_E_ARG && n == want.size();
            for (size_t i = 0; i + 1 < want.size(); i++) kept = kept && small.p[i] == 0x5A;
            expect(kept, "host short cap", name);
        }
    }
    // every two-way cut, each part in a block of its own
    if (cuts)
        for (size_t p = 0; p <= len; p++) {
            Block a(p), b(len - p);
            if (p) memcpy(a.p, text.p, p);
            if (len - p) memcpy(b.p, text.p + p, len - p);
            std::vector<uint8_t> got = parse_model(a.p, p, (uint32_t)(p & 15u), 0);
            const std::vector<uint8_t> second = parse_model(b.p, len - p, (uint32_t)((p * 5 + 1) & 15u), (uint32_t)(got.size() & 15u));
            got.insert(got.end(), second.begin(), second.end());
            expect(got == want, "cut", name);
        }

    // the writer on the text's bits
    printf("%s %zu %016llx", name.c_str(), want.size(), (unsigned long long)fnv(want.data(), want.size()));
    Block bits(want.size());
    if (!want.empty()) memcpy(bits.p, want.data(), want.size());
    const size_t n = want.size();
    const uint64_t lbs[] = {0, 1, 7, 16, 64, n, n + 1};
    for (uint64_t lb : lbs) {
        const std::vector<uint8_t> loop = write_loop(bits.p, n, lb);
        expect(loop.size() == wt_text_len(n, lb), "text length", name);
        for (uint32_t shift = 0; shift < 16; shift++) {
            bool bad = true;
            expect(write_model(bits.p, n, lb, shift, &bad) == loop && !bad, "write", name);
        }
        size_t got_len = 0;
        Block out(loop.size());
        expect(rv_witness_write(bits.p, n, lb, (char*)out.p, loop.size(), &got_len) == RV_OK && got_len == loop.size() && same(out.p, loop),
               "host write", name);
        expect(parse_model(out.p, loop.size(), 3, 9) == want, "write then parse", name);
        printf(" %016llx", (unsigned long long)fnv(loop.data(), loop.size()));
    }
    printf("\n");
    // a bit above 1, first, last and in the middle: the flag, from the lane that meets it
    for (size_t at : {(size_t)0, n / 2, n ? n - 1 : 0}) {
        if (!n) break;
        bits.p[at] = 2;
        bool bad = false;
        (void)write_model(bits.p, n, 7, 5, &bad);
        size_t got_len = 0;
        Block out(wt_text_len(n, 7));
        expect(bad && rv_witness_write(bits.p, n, 7, (char*)out.p, out.n, &got_len) == RV_E_ARG, "bad bit", name);
        bits.p[at] = want[at];
    }
}

int main(int argc, char** argv) {
    bool cuts = false;
    for (int i = 1; i < argc; i++) {
        if (!strcmp(argv[i], "--cuts")) cuts = true;
        else run_file(argv[i], cuts);
    }
    printf("checks %llu\nbad %llu\n", (unsigned long long)g_checks, (unsigned long long)g_bad);
    return g_bad ? 1 : 0;
}
