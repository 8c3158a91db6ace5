// The windowed Bristol reader (rv_bristol_reader_*) without a GPU: the functions of reverie_amd/csrc/bristol_dev.h -- what a lane, a
// line and the state between the windows do -- with the kernels of bristol_dev.hip written as plain loops in the kernels' order.
// Every window, every carry and every work array is a heap block of exactly its bytes, so AddressSanitizer sees a read outside
// text[0, len).  bristol.cpp is linked in as the answer: records, codes, info, and (one line at a time) which line is the first bad one.
//
//   model CASE...                      every case cut in two (every position up to 2100 bytes; chosen and seeded positions above)
//         --fixed CASE...              fed 1, 7, 8 and 9 bytes at a time
//         --mutations N CASE           N seeded byte mutations, each at seeded random cuts
//         --resume CASE                a reader placed above 2^32
// A case file: u32 format, u32 has_expected, u32 n_expected, the expected bytes, the text.  Prints "cases N" and "bad M".
#include <stdio.h>
#include <stdlib.h>

#include <algorithm>
#include <string>

#include "bristol_dev.h"

using namespace rv;

namespace {
constexpr uint32_t TB = 256;
constexpr uint64_t NO_ERR = ~0ull;
long g_cases = 0, g_bad = 0;

struct Case {
    std::string name;
    int fmt = 0;
    bool has_exp = false;
    std::vector<uint8_t> exp;
    std::vector<char> text;
};

// ---- the kernels of one buffer, as loops (gates_run of bristol_dev.hip) ----
struct Words {
    uint64_t err = NO_ERR, lines = 0, ops = 0, cls[4] = {0, 0, 0, 0}, tail = 0, lf_end = 0;
};
void lane_masks(const uint8_t* buf, uint64_t bytes, uint64_t at, uint32_t& lf, uint32_t& tok) {
    lf = tok = 0;
    if (at < bytes) br_classify_bytes(buf + at, buf, buf + bytes, lf, tok);
}
Words model_gates(const uint8_t* buf, uint64_t bytes, const BrWindowLaunch& l, uint64_t n_wires, const uint8_t* expected, uint64_t* out, uint64_t cap_ops) {
    Words w;
    const uint8_t* hi = buf + bytes;
    const uint32_t n_tiles = (uint32_t)std::max<uint64_t>(1, (bytes + BRISTOL_TILE_BYTES - 1) / BRISTOL_TILE_BYTES);
    const uint64_t cap = br_line_cap(bytes, l.want);
    std::vector<uint32_t> tkey(n_tiles), tmeta(n_tiles), tin(n_tiles), tbase(n_tiles), line_off(cap), cnt(cap), first(cap);
    // k_bp_tiles<false, true>
    for (uint32_t t = 0; t < n_tiles; t++) {
        uint32_t prev = 0, total = 0, cond = 0, lf_end = 0;
        for (uint32_t lane = 0; lane < TB; lane++) {
            const uint64_t at = (uint64_t)t * BRISTOL_TILE_BYTES + lane * 16;
            uint32_t lf, tok;
            lane_masks(buf, bytes, at, lf, tok);
            const uint32_t key = br_lane_key(lane, lf, tok);
            total += (uint32_t)__builtin_popcount(br_lane_starts(lf, tok, prev ? (prev & 1u) : 0u));
            if (!prev && (lf | tok)) cond = br_lane_cond(lf, tok);
            lf_end = std::max(lf_end, br_lane_lf_end(lf, at));
            prev = std::max(prev, key);
        }
        tkey[t] = br_tile_key(t, prev);
        tmeta[t] = total | (cond << 31);
        w.lf_end = std::max<uint64_t>(w.lf_end, lf_end);
    }
    // the keys' exclusive max-scan, k_bp_counts, the counts' exclusive sum
    uint32_t run = 0;
    for (uint32_t t = 0; t < n_tiles; t++) tin[t] = run, run = std::max(run, tkey[t]);
    w.tail = run;
    uint32_t sum = 0;
    for (uint32_t t = 0; t < n_tiles; t++) tbase[t] = sum, sum += br_tile_count(tmeta[t], tin[t]);
    w.lines = sum;
    const BrTake tk = br_take(w.lines, (uint32_t)w.tail, l.at_end, l.want);
    const uint64_t n = std::min(tk.take, cap);
    // k_bp_tiles<true, false>
    for (uint32_t t = 0; t < n_tiles; t++) {
        uint32_t prev = 0;
        uint64_t idx = tbase[t];
        for (uint32_t lane = 0; lane < TB; lane++) {
            const uint64_t at = (uint64_t)t * BRISTOL_TILE_BYTES + lane * 16;
            uint32_t lf, tok;
            lane_masks(buf, bytes, at, lf, tok);
            const uint32_t starts = br_lane_starts(lf, tok, prev ? (prev & 1u) : (tin[t] & 1u));
            for (int k = 0; k < 16; k++)
                if ((starts >> k) & 1u) {
                    if (idx < n) line_off[idx] = (uint32_t)(at + k);
                    idx++;
                }
            prev = std::max(prev, br_lane_key(lane, lf, tok));
        }
    }
    // k_bp_validate
    const uint64_t grid = std::max<uint64_t>(1, (cap + TB - 1) / TB) * TB;
    for (uint64_t i = 0; i < grid; i++) {
        BrLine r{0, -1, 0};
        if (i < n) r = br_validate(buf + line_off[i], hi, n_wires);
        else if (tk.short_file && i == tk.found) r.code = RV_E_BAD_OP;
        if (i < cap) cnt[i] = (uint32_t)r.recs;
        if (r.code) w.err = std::min(w.err, i << 8 | (uint64_t)r.code);
        else if (r.cl >= 0) w.cls[r.cl] += r.recs;
    }
    for (uint64_t i = 0; i < cap; i++) first[i] = (uint32_t)w.ops, w.ops += cnt[i];
    // k_bp_emit, k_bp_inputs, k_bp_asserts
    if (out && w.err == NO_ERR && l.n_inputs + w.ops + (tk.last ? 2 * l.n_pairs : 0) <= cap_ops) {
        for (uint64_t i = 0; i < n; i++) br_emit(buf + line_off[i], hi, out, l.n_inputs + first[i]);
        for (uint64_t k = 0; k < l.n_inputs; k++) br_emit_input(out, k, k);
        if (tk.last)
            for (uint64_t k = 0; k < l.n_pairs; k++) br_emit_pair(out, l.n_inputs + w.ops + 2 * k, n_wires, l.n_pairs, k, expected[k]);
    }
    return w;
}

// ---- the reader (rv_bristol_reader_feed of bristol.inc, host memory in place of the arena) ----
struct Reader {
    BrWindowState s;
    std::vector<uint8_t> expected;
    uint8_t* carry = nullptr;
    ~Reader() { delete[] carry; }
    uint64_t held() const { return s.have_header ? s.carry : s.head.size(); }  // (the capacity bound's `held`)
    int feed(const char* text, size_t len, uint64_t* out, uint64_t cap_ops, rv_bristol_piece* piece) {
        if (s.code || len > s.file_len - s.fed) return RV_E_ARG;
        const bool had_header = s.have_header;
        const BrHeadMark mark = br_window_mark(s);
        if (br_window_complete(s)) {
            br_window_skip(s, len, piece);
            return RV_OK;
        }
        size_t taken = 0, host_len = 0;
        if (!had_header) {
            bool ready = br_window_head_scan(s, s.fed);
            while (!ready) {
                const size_t need = br_window_head_need(s, len - taken);
                if (!need) break;
                s.head.insert(s.head.end(), text + taken, text + taken + need);
                taken += need;
                ready = br_window_head_scan(s, s.fed + taken);
            }
            if (!ready) {
                br_window_skip(s, len, piece);
                return RV_OK;
            }
            if (int rc = br_window_header(s)) return rc;
            host_len = s.head.size() - s.gates_offset;
        }
        const uint64_t bytes = s.carry + host_len + (len - taken);
        const BrWindowLaunch l = br_window_launch(s, len);
        uint8_t* buf = new uint8_t[bytes];
        if (s.carry) memcpy(buf, carry, s.carry);
        if (host_len) memcpy(buf + s.carry, s.head.data() + s.gates_offset, host_len);
        if (len > taken) memcpy(buf + s.carry + host_len, text + taken, len - taken);
        const bool may_finish = br_line_cap(bytes, l.want) == l.want;
        BrWindowLaunch lk = l;
        if (!may_finish) lk.n_pairs = 0;
        const Words w = model_gates(buf, bytes, lk, s.info.n_wires, expected.data(), out, cap_ops);
        BrWindowResult res;
        if (w.err != NO_ERR) res.code = (int)(w.err & 0xFF);
        else {
            const BrTake t = br_take(w.lines, (uint32_t)w.tail, l.at_end, l.want);
            res.n_lines = t.take, res.last = t.last, res.gate_ops = w.ops;
            res.n_and = w.cls[0], res.n_xor = w.cls[1], res.n_inv = w.cls[2], res.n_other = w.cls[3];
            res.carry_from = w.lf_end;
        }
        const uint64_t carry_bytes = res.code ? 0 : br_window_carry(l, res, bytes);
        const int rc = br_window_done(s, len, bytes, l, res, out == nullptr, cap_ops, piece);
        if (rc) {
            if (rc == RV_E_ARG && !s.code && !had_header) br_window_rollback(s, mark);
            delete[] buf;
            return rc;
        }
        uint8_t* nc = carry_bytes ? new uint8_t[carry_bytes] : nullptr;
        if (carry_bytes) memcpy(nc, buf + res.carry_from, carry_bytes);
        delete[] carry;
        carry = nc;
        delete[] buf;
        s.head = std::vector<char>();
        return RV_OK;
    }
};

// ---- the answer ----
struct Answer {
    int rc = 0;
    std::vector<uint8_t> recs;
    rv_bristol_info info = {};
    uint64_t header_at = 0;         // bytes fed when the header is complete
    std::vector<uint64_t> final_at;  // bytes fed when gate line i < n_gates is final
    uint64_t error_at = 0;          // bytes fed when the code is due
    uint64_t n_inputs = 0;          // the header's (0: it has a code)
};
int host(const Case& c, const std::vector<char>& text, std::vector<uint8_t>* recs, rv_bristol_info* info) {
    rv_op* ops = nullptr;
    size_t n = 0;
    const int rc = rv_bristol_parse(text.empty() ? "" : text.data(), text.size(), c.fmt, c.has_exp ? (c.exp.empty() ? (const uint8_t*)"" : c.exp.data()) : nullptr,
                                    c.exp.size(), &ops, &n, info);
    if (!rc && recs) recs->assign((const uint8_t*)ops, (const uint8_t*)ops + n * sizeof(rv_op));
    if (!rc) free(ops);
    return rc;
}
Answer answer(const Case& c, const std::vector<char>& text) {
    Answer a;
    const uint64_t len = text.size();
    a.rc = host(c, text, &a.recs, &a.info);
    // the header is complete behind the fourth whole non-blank line, or at the file's end
    a.header_at = len;
    int lines = 0;
    bool token = false;
    for (uint64_t i = 0; i < len && lines < 4; i++) {
        if (text[i] == '\n') {
            lines += token, token = false;
            if (lines == 4) a.header_at = i + 1;
        } else if (text[i] != ' ' && text[i] != '\t' && text[i] != '\r') token = true;
    }
    rv_bristol_info h;
    size_t off = 0;
    const int hrc = rv_internal_bristol_header(len ? text.data() : "", len, len, c.fmt, c.has_exp, c.exp.size(), &h, &off);
    a.error_at = a.header_at;
    if (hrc) return a;
    a.n_inputs = h.n_inputs;
    // the gate lines; the host's code for each alone (a text of one gate line and as many wires) names the first bad one
    int first_code = 0;
    bool found_bad = false;
    uint64_t p = off, short_at = len;
    for (uint64_t i = 0; i < h.n_gates && p < len;) {
        uint64_t e = p;
        while (e < len && text[e] != '\n') e++;
        bool blank = true;
        for (uint64_t k = p; k < e; k++) blank &= text[k] == ' ' || text[k] == '\t' || text[k] == '\r';
        const uint64_t fin = std::max<uint64_t>(e < len ? e + 1 : len, a.header_at);
        if (!blank) {
            a.final_at.push_back(fin);
            if (!found_bad) {
                Case one;
                one.fmt = 1;
                char head[64];
                const int hn = snprintf(head, sizeof head, "1 %llu\n1 0\n1 0\n", (unsigned long long)h.n_wires);
                std::vector<char> t(head, head + hn);
                t.insert(t.end(), text.begin() + p, text.begin() + e);
                first_code = host(one, t, nullptr, nullptr);
                if (first_code) found_bad = true, a.error_at = fin;
            }
            i++;
        }
        p = e < len ? e + 1 : len;
    }
    if (!found_bad) a.error_at = a.final_at.size() < h.n_gates ? short_at : (a.final_at.empty() ? a.header_at : a.final_at.back());
    if (a.rc && found_bad && first_code != a.rc) printf("MODEL %s: the lines alone say %d, the text %d\n", c.name.c_str(), first_code, a.rc), g_bad++;
    return a;
}

// one text fed at the given cuts (ascending offsets inside the text; the feeds are the ranges between them)
void run(const Case& c, const std::vector<char>& text, const Answer& a, std::vector<uint64_t> cuts, bool scan_some) {
    g_cases++;
    const uint64_t len = text.size();
    cuts.push_back(len);
    Reader r;
    br_window_begin(r.s, len, c.fmt, c.has_exp, c.exp.size());
    r.expected = c.exp;
    std::vector<uint8_t> got;
    std::vector<bool> known;
    uint64_t at = 0, lines = 0, ops = 0;
    int rc = 0;
    auto fail = [&](const char* what, uint64_t x, uint64_t y) {
        printf("FAIL %s: %s (%llu, %llu) at %llu of %llu\n", c.name.c_str(), what, (unsigned long long)x, (unsigned long long)y, (unsigned long long)at,
               (unsigned long long)len);
        g_bad++;
    };
    for (size_t k = 0; k < cuts.size() && !rc; k++) {
        const uint64_t n = cuts[k] - at;
        char* win = new char[n];  // exactly the feed's bytes
        if (n) memcpy(win, text.data() + at, n);
        const uint64_t bound = (r.s.inputs_out ? 0 : a.n_inputs) + (r.held() + n) / 6 + 1 + 2 * c.exp.size();
        const bool scan = scan_some && (k & 1);
        rv_bristol_piece piece;
        uint64_t* out = nullptr;
        if (!scan && bound < (1u << 24)) {
            // the capacity rule first: one record too few changes nothing
            out = new uint64_t[3 * bound];
            rc = r.feed(win, n, out, bound, &piece);
        } else {
            rc = r.feed(win, n, nullptr, 0, &piece);
        }
        at = cuts[k];
        if (!rc) {
            const uint64_t due = at < a.header_at ? 0 : (uint64_t)(std::upper_bound(a.final_at.begin(), a.final_at.end(), at) - a.final_at.begin());
            if (piece.first_line != lines || piece.first_line + piece.n_lines != due) fail("lines delivered", piece.first_line + piece.n_lines, due);
            if (piece.first_op != ops) fail("first_op", piece.first_op, ops);
            if (piece.n_ops > bound) fail("the bound", piece.n_ops, bound);
            lines += piece.n_lines, ops += piece.n_ops;
            if (out) got.insert(got.end(), (uint8_t*)out, (uint8_t*)out + piece.n_ops * 24);
            else got.insert(got.end(), piece.n_ops * 24, 0);
            known.insert(known.end(), piece.n_ops, out != nullptr);  // (a scan feed's records are counted, not compared)
        }
        delete[] out;
        delete[] win;
    }
    if (rc != a.rc) return fail("code", (uint64_t)rc, (uint64_t)a.rc);
    if (rc) {
        if (at != std::min<uint64_t>(*std::lower_bound(cuts.begin(), cuts.end(), a.error_at), len)) fail("the feed of the code", at, a.error_at);
        rv_bristol_piece piece;
        if (r.feed("", 0, nullptr, 0, &piece) != RV_E_ARG || br_window_finish(r.s, nullptr) != RV_E_ARG) fail("after a code", 0, 0);
        return;
    }
    rv_bristol_info info;
    if (br_window_finish(r.s, &info) != RV_OK) return fail("finish", 0, 0);
    if (memcmp(&info, &a.info, sizeof info)) fail("info", info.n_and, a.info.n_and);
    if (got.size() != a.recs.size()) return fail("record count", got.size() / 24, a.recs.size() / 24);
    for (size_t i = 0; i < got.size(); i += 24)
        if (known[i / 24] && memcmp(&got[i], &a.recs[i], 24)) return fail("record", i / 24, 0);
}

Case load(const char* path) {
    Case c;
    c.name = path;
    FILE* f = fopen(path, "rb");
    if (!f) exit(2);
    uint32_t h[3];
    if (fread(h, 4, 3, f) != 3) exit(2);
    c.fmt = (int)h[0], c.has_exp = h[1] != 0;
    c.exp.resize(h[2]);
    if (h[2] && fread(c.exp.data(), 1, h[2], f) != h[2]) exit(2);
    char buf[65536];
    for (size_t n; (n = fread(buf, 1, sizeof buf, f)) > 0;) c.text.insert(c.text.end(), buf, buf + n);
    fclose(f);
    return c;
}
uint64_t g_rng = 0x9E3779B97F4A7C15ull;
uint64_t rnd() {
    g_rng ^= g_rng << 13, g_rng ^= g_rng >> 7, g_rng ^= g_rng << 17;
    return g_rng;
}

void two_cuts(const Case& c) {
    const Answer a = answer(c, c.text);
    const uint64_t len = c.text.size();
    std::vector<uint64_t> at;
    if (len <= 2100) {
        for (uint64_t k = 0; k <= len; k++) at.push_back(k);
    } else {
        rv_bristol_info h;
        size_t off = 0;
        (void)rv_internal_bristol_header(c.text.data(), len, len, c.fmt, 0, 0, &h, &off);
        auto near = [&](uint64_t x) {
            for (int d = -2; d <= 2; d++)
                if ((int64_t)x + d >= 0 && x + d <= len) at.push_back(x + d);
        };
        near(0), near(len), near(off), near(a.header_at);
        // a tile edge of the second feed's buffer lies a whole number of tiles behind the cut, and behind the line start before it
        for (uint64_t t = BRISTOL_TILE_BYTES; t < len; t += BRISTOL_TILE_BYTES) near(t), near(off + t), near(len - t);
        for (int k = 0; k < 40; k++) at.push_back(rnd() % (len + 1));
        std::sort(at.begin(), at.end());
        at.erase(std::unique(at.begin(), at.end()), at.end());
    }
    for (uint64_t k : at) run(c, c.text, a, {k}, (k & 3) == 3);
    printf("cuts %zu %s\n", at.size(), c.name.c_str());
}
void fixed(const Case& c) {
    const Answer a = answer(c, c.text);
    int n = 0;
    for (uint64_t step : {1, 7, 8, 9}) {
        std::vector<uint64_t> cuts;
        for (uint64_t k = step; k < c.text.size(); k += step) cuts.push_back(k);
        run(c, c.text, a, cuts, step == 7), n++;
    }
    printf("fixed %d %s\n", n, c.name.c_str());
}
void mutations(const Case& c, int n) {
    for (int m = 0; m < n; m++) {
        std::vector<char> t = c.text;
        const int edits = 1 + (int)(rnd() % 3);
        for (int e = 0; e < edits && !t.empty(); e++) {
            const uint64_t at = rnd() % t.size();
            static const char pool[] = "0123456789 \n\tXANDORIVEQWM\r-x\x00";
            switch (rnd() % 4) {
            case 0: t[at] = pool[rnd() % (sizeof pool)]; break;
            case 1: t.erase(t.begin() + at); break;
            case 2: t.insert(t.begin() + at, pool[rnd() % (sizeof pool)]); break;
            default: t.resize(at); break;
            }
        }
        const Answer a = answer(c, t);
        std::vector<uint64_t> cuts;
        for (int k = (int)(rnd() % 4); k > 0 && !t.empty(); k--) cuts.push_back(rnd() % (t.size() + 1));
        std::sort(cuts.begin(), cuts.end());
        run(c, t, a, cuts, (m & 7) == 7);
    }
    printf("mutations %d\n", n);
}
// The case's gate lines as the LAST lines of a file of more than 2^32 bytes: the header names 2^29 lines more, the reader is placed
// behind them (the hook's steps: the header lines alone, then the position), and the tail is fed in two pieces at every cut.
void resume(const Case& c) {
    const Answer a = answer(c, c.text);
    rv_bristol_info h;
    size_t off = 0;
    if (a.rc || rv_internal_bristol_header(c.text.data(), c.text.size(), c.text.size(), c.fmt, 0, 0, &h, &off)) exit(2);
    const uint64_t before = 1ull << 29, file_len = (9ull << 32) + 12345, op0 = (1ull << 33) + 7;
    char head[128];
    const int hn = snprintf(head, sizeof head, "%llu %llu\n1 %llu\n1 %llu\n", (unsigned long long)(h.n_gates + before), (unsigned long long)h.n_wires,
                            (unsigned long long)h.n_inputs, (unsigned long long)h.n_outputs);
    const std::vector<char> tail(c.text.begin() + off, c.text.end());
    int n = 0;
    for (uint64_t cut = 0; cut <= tail.size(); cut += 1 + cut / 64, n++) {
        g_cases++;
        Reader r;
        br_window_begin(r.s, file_len, 1, c.has_exp, c.exp.size());
        r.expected = c.exp;
        rv_bristol_piece piece;
        int rc = r.feed(head, (size_t)hn, nullptr, 0, &piece);
        if (rc || r.s.have_header || br_window_header(r.s)) exit(2);
        r.s.head = std::vector<char>();
        r.s.fed = file_len - tail.size(), r.s.lines_done = before, r.s.ops_done = op0, r.s.inputs_out = true;
        std::vector<uint64_t> out(3 * (tail.size() / 6 + 2 + 2 * c.exp.size()));
        std::vector<uint8_t> got;
        uint64_t ops = op0, lines = before;
        for (int k = 0; k < 2 && !rc; k++) {
            const uint64_t lo = k ? cut : 0, hi = k ? tail.size() : cut;
            char* win = new char[hi - lo];
            if (hi > lo) memcpy(win, tail.data() + lo, hi - lo);
            rc = r.feed(win, hi - lo, out.data(), out.size() / 3, &piece);
            delete[] win;
            if (!rc && (piece.first_op != ops || piece.first_line != lines)) printf("FAIL resume: ordinals\n"), g_bad++;
            ops += piece.n_ops, lines += piece.n_lines;
            if (!rc) got.insert(got.end(), (uint8_t*)out.data(), (uint8_t*)out.data() + piece.n_ops * 24);
        }
        rv_bristol_info info;
        const size_t skip = (size_t)h.n_inputs * 24;
        if (rc || br_window_finish(r.s, &info) || lines != before + h.n_gates || got.size() + skip != a.recs.size() ||
            memcmp(got.data(), a.recs.data() + skip, got.size()))
            printf("FAIL resume at cut %llu: rc %d\n", (unsigned long long)cut, rc), g_bad++;
    }
    printf("resume %d\n", n);
}
}  // namespace

int main(int argc, char** argv) {
    int mode = 0;
    for (int i = 1; i < argc; i++) {
        const std::string s = argv[i];
        if (s == "--fixed") mode = 1;
        else if (s == "--mutations") mode = 2;
        else if (s == "--resume") mode = 3;
        else if (mode == 0) two_cuts(load(argv[i]));
        else if (mode == 1) fixed(load(argv[i]));
        else if (mode == 2) {
            const int n = atoi(argv[i]);
            mutations(load(argv[++i]), n);
        } else resume(load(argv[i]));
    }
    printf("cases %ld\nbad %ld\n", g_cases, g_bad);
    return g_bad ? 1 : 0;
}
