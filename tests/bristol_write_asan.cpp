// Stand-alone host program around the Bristol writer's per-record code (reverie_amd/csrc/bristol_write.h), built with
// -fsanitize=address,undefined by tests/test_bristol_write_host.py.  The code, the length and the bytes of a record's line, and the
// header lines, are the functions the kernels of bristol_write.hip call; here they run as plain loops in the kernels' order: the
// lengths pass with its four reductions (an Input's place in the leading run read off its predecessor, as the kernel reads it), an
// exclusive sum, then one emit per group of 256 records into an image of exactly the kernel's LDS size, copied from there into a
// heap block of exactly the text's bytes -- so a line that is longer than its length, or an image that overflows, is a sanitizer
// report.  The answer is compared with rv_bristol_write (bristol.cpp, linked in) on the same records.
//
//   bristol_write_asan FILE...            every case file whole
//   bristol_write_asan --cuts FILE...     ... and, for the files that follow, the windowed rule (rv_bristol_writer_*) for every pair
//                                         of cut points: three feeds, feeds of 0 records included
// A case file: three little-endian u64 (n_wires, 0 = derive; n_outputs; n_ops), then n_ops 24-byte rv_op records.
// Prints one line per file (name, code, length, FNV-1a 64 of the text in hex), "cuts K" per file cut (K cuttings), and "bad K" at
// the end (K mismatches).
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <string>
#include <vector>

#include "bristol_write.h"

using namespace rv;

struct Case {
    uint64_t n_wires = 0, n_outputs = 0;
    std::vector<rv_op> ops;
};
struct Answer {
    int code = 0;
    std::vector<uint8_t> text;
};

static void words(const rv_op& o, uint64_t w[3]) { memcpy(w, &o, sizeof o); }
static bool is_input(const rv_op& o) { return o.domain == RV_DOM_GF2 && o.opcode == RV_OP_INPUT; }

// one launch of the three steps over ops[0, n): a whole list (J.whole) or one feed.  -> the code; the bytes into `out` (appended)
static int launch(const rv_op* ops, size_t n, const BwJob& J, std::vector<uint8_t>& out) {
    constexpr uint32_t TB = BRISTOL_WRITE_TILE, IMAGE = 16 + BW_MAX_HEADER + TB * BW_MAX_LINE + 16;
    auto in_run = [&](size_t i) { return J.whole ? is_input(ops[i]) && (i == 0 || is_input(ops[i - 1])) : J.first_op + i < J.n_inputs; };
    // 1. lengths
    std::vector<uint32_t> lens(n);
    uint64_t err = BW_NO_ERR, total = 0, need = 0, run = n;
    for (size_t i = 0; i < n; i++) {
        uint64_t w[3], nd;
        words(ops[i], w);
        const int code = bw_judge(w, J.first_op + i, in_run(i), J.n_wires, lens[i], nd);
        if (code) err = std::min(err, (uint64_t)(J.first_op + i) << 8 | (uint64_t)code);
        if (J.whole && !is_input(ops[i])) run = std::min<uint64_t>(run, i);
        total += lens[i], need = std::max(need, nd);
    }
    if (err != BW_NO_ERR) return (int)(err & 0xFFu);
    const uint64_t inputs = J.whole ? run : J.n_inputs, wires = J.n_wires ? J.n_wires : std::max(need, inputs);
    if (const int code = bw_header_code(wires, inputs, J.n_outputs)) return code;
    const uint64_t gates = J.total_ops - inputs;
    const uint32_t head = J.header ? bw_header_len(gates, wires, inputs, J.n_outputs) : 0;
    // 2. scan
    std::vector<uint32_t> offs(n);
    uint32_t acc = 0;
    for (size_t i = 0; i < n; i++) offs[i] = acc, acc += lens[i];
    // 3. emit: the text is a heap block of exactly its bytes
    const size_t bytes = head + total;
    uint8_t* text = (uint8_t*)malloc(bytes ? bytes : 1);
    const size_t grid = std::max<size_t>(1, (n + TB - 1) / TB);
    for (size_t blk = 0; blk < grid; blk++) {
        uint8_t* raw = (uint8_t*)malloc(IMAGE);
        const size_t first = blk * TB, mine = std::min<size_t>(TB, n > first ? n - first : 0);
        const uint64_t g0 = blk ? head + (uint64_t)offs[first] : 0;
        const uint32_t sh = (uint32_t)(g0 & 15u);  // (as if the text began at an aligned address)
        uint64_t end = head;
        if (blk == 0 && head) bw_header(gates, wires, inputs, J.n_outputs, [&](uint32_t k, uint8_t v) { raw[sh + k] = v; });
        for (size_t t = 0; t < mine; t++) {
            const size_t i = first + t;
            uint64_t w[3], nd;
            uint32_t l;
            words(ops[i], w);
            (void)bw_judge(w, J.first_op + i, in_run(i), J.n_wires, l, nd);
            const uint64_t at = head + (uint64_t)offs[i];
            if (l) {
                uint8_t* dst = raw + sh + (uint32_t)(at - g0);
                bw_emit(w, [&](uint32_t k, uint8_t v) { dst[k] = v; });
            }
            if (t == mine - 1) end = at + l;
        }
        const uint32_t span = sh + (uint32_t)(end - g0);
        for (uint32_t c = sh; c < span; c++) text[g0 - sh + c] = raw[c];
        free(raw);
    }
    out.insert(out.end(), text, text + bytes);
    free(text);
    return 0;
}

static Answer whole(const Case& c) {
    Answer A;
    BwJob J = {};
    J.total_ops = c.ops.size(), J.n_wires = c.n_wires, J.n_outputs = c.n_outputs, J.whole = 1, J.header = 1;
    A.code = launch(c.ops.data(), c.ops.size(), J, A.text);
    return A;
}

static Answer host(const Case& c) {
    Answer A;
    char* text = nullptr;
    size_t len = 0;
    A.code = rv_bristol_write(c.ops.data(), c.ops.size(), c.n_wires, c.n_outputs, &text, &len);
    if (!A.code) A.text.assign((uint8_t*)text, (uint8_t*)text + len);
    free(text);
    return A;
}

// rv_bristol_writer_*: begin's checks, then the feeds [0, c1), [c1, c2), [c2, n); the first code ends it
static Answer windowed(const Case& c, uint64_t n_inputs, uint64_t n_wires, size_t c1, size_t c2) {
    Answer A;
    const size_t n = c.ops.size();
    if (n_inputs > n || (!n_wires && n)) return A.code = RV_E_ARG, A;
    if ((A.code = bw_header_code(n_wires, n_inputs, c.n_outputs))) return A;
    const size_t cuts[4] = {0, c1, c2, n};
    for (int f = 0; f < 3 && !A.code; f++) {
        BwJob J = {};
        J.first_op = cuts[f], J.total_ops = n, J.n_inputs = n_inputs, J.n_wires = n_wires, J.n_outputs = c.n_outputs, J.header = f == 0;
        A.code = launch(c.ops.data() + cuts[f], cuts[f + 1] - cuts[f], J, A.text);
    }
    if (A.code) A.text.clear();
    return A;
}

static uint64_t fnv(const std::vector<uint8_t>& v) {
    uint64_t h = 0xcbf29ce484222325ull;
    for (uint8_t b : v) h = (h ^ b) * 0x100000001b3ull;
    return h;
}

int main(int argc, char** argv) {
    int bad = 0;
    bool cuts = false;
    for (int k = 1; k < argc; k++) {
        if (!strcmp(argv[k], "--cuts")) {
            cuts = true;
            continue;
        }
        FILE* f = fopen(argv[k], "rb");
        if (!f) return 2;
        Case c;
        uint64_t head[3];
        if (fread(head, 8, 3, f) != 3) return 2;
        c.n_wires = head[0], c.n_outputs = head[1];
        c.ops.resize(head[2]);
        if (head[2] && fread(c.ops.data(), sizeof(rv_op), head[2], f) != head[2]) return 2;
        fclose(f);
        const Answer want = host(c), got = whole(c);
        if (want.code != got.code || want.text != got.text) bad++, printf("MISMATCH whole %s\n", argv[k]);
        const char* base = strrchr(argv[k], '/');
        printf("%s %d %zu %016llx\n", base ? base + 1 : argv[k], got.code, got.text.size(), (unsigned long long)fnv(got.text));
        if (!cuts) continue;
        // what the whole-list call derives (for a list with a code: the run of Inputs, and a wire count no index reaches)
        size_t n_in = 0;
        while (n_in < c.ops.size() && is_input(c.ops[n_in])) n_in++;
        uint64_t wires = c.n_wires;
        if (!wires) {
            wires = n_in;
            for (size_t i = 0; i < c.ops.size(); i++) {
                uint64_t w[3], nd;
                uint32_t l;
                words(c.ops[i], w);
                if (bw_judge(w, i, i < n_in, 0, l, nd)) {
                    wires = 1ull << 32;
                    break;
                }
                wires = std::max(wires, nd);
            }
        }
        size_t done = 0;
        for (size_t c1 = 0; c1 <= c.ops.size(); c1++)
            for (size_t c2 = c1; c2 <= c.ops.size(); c2++, done++) {
                const Answer w = windowed(c, n_in, wires, c1, c2);
                if (w.code != want.code || w.text != want.text) bad++, printf("MISMATCH cuts %zu %zu %s (%d vs %d)\n", c1, c2, argv[k], w.code, want.code);
            }
        printf("cuts %zu\n", done);
    }
    printf("bad %d\n", bad);
    return bad ? 1 : 0;
}
