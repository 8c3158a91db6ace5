// Stand-alone host program around walk_proof (reverie_amd/csrc/verify_dev.h), built with -fsanitize=address,undefined by
// tests/test_verify_device_host.py: the walker that k_parse_proof runs on the GPU is this same function, and here every byte
// string it is given lives in a heap block of exactly its length, so a load past the bytes is a sanitizer report.
//
//   verify_walk_asan FILE...                 every file whole, as bincode(Proof) and -- cut into its four sections -- as sections
//   verify_walk_asan --prefixes FILE         ... and every prefix of FILE, and FILE with each of its four counts set to
//                                            0, 39, 41 and 2^63
// Prints one line per walk: what, length, status, a 64-bit FNV-1a of the table (the test compares them with the library's hook).
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

#include "verify_dev.h"

using namespace rv;

static uint64_t fnv(const uint64_t* t) {
    uint64_t h = 0xCBF29CE484222325ull;
    for (int i = 0; i < VW_WORDS; i++)
        for (int b = 0; b < 8; b++) h = (h ^ ((t[i] >> (8 * b)) & 0xFF)) * 0x100000001B3ull;
    return h;
}

// the walk over an exact-size heap copy of bytes[0, len)
static int walk(const char* what, const uint8_t* bytes, size_t len, int framing, const uint64_t* lens, uint64_t* table, bool print = true) {
    uint8_t* copy = (uint8_t*)malloc(len ? len : 1);
    if (len) memcpy(copy, bytes, len);
    memset(table, 0, VW_WORDS * 8);
    const int status = walk_proof(len ? copy : copy + 1, len, framing, lens, table);
    free(copy);
    if (print) printf("%s %zu %d %016llx\n", what, len, status, (unsigned long long)fnv(table));
    return status;
}

int main(int argc, char** argv) {
    bool prefixes = false;
    int bad = 0;
    for (int a = 1; a < argc; a++) {
        if (!strcmp(argv[a], "--prefixes")) {
            prefixes = true;
            continue;
        }
        FILE* f = fopen(argv[a], "rb");
        if (!f) return 2;
        std::vector<uint8_t> d;
        uint8_t buf[4096];
        for (size_t n; (n = fread(buf, 1, sizeof buf, f)) > 0;) d.insert(d.end(), buf, buf + n);
        fclose(f);
        std::vector<uint64_t> t(VW_WORDS), ts(VW_WORDS);
        if (walk("proof", d.data(), d.size(), VW_FRAMING_PROOF, nullptr, t.data()) != VW_OK) continue;
        // the four sections of a proof that walked: records of a domain run from its first keys' omit byte to its count of 216
        std::vector<uint8_t> sec;
        uint64_t lens[4];
        for (int dom = 0; dom < 2; dom++) {
            const uint64_t on0 = t[VW_REC + 8 * VW_N_ON * dom + VW_KEYS] - 1, pre0 = t[VW_PRE + dom];
            lens[2 * dom] = pre0 - 8 - on0;
            lens[2 * dom + 1] = (uint64_t)VW_N_PRE * 48;
            sec.insert(sec.end(), d.begin() + on0, d.begin() + pre0 - 8);
            sec.insert(sec.end(), d.begin() + pre0, d.begin() + pre0 + lens[2 * dom + 1]);
        }
        if (walk("sections", sec.data(), sec.size(), VW_FRAMING_SECTIONS, lens, ts.data()) != VW_OK) bad++;
        // ... hold the same records, 40 bytes further to the front in the first domain, 56 in the second
        for (int k = 0; k < 2 * VW_N_ON; k++)
            for (int w = 0; w < 8; w++) {
                const bool off = w == VW_KEYS || w == VW_OFF_REC || w == VW_OFF_CORR || w == VW_OFF_IN;
                const uint64_t shift = off ? (k < VW_N_ON ? 40 : 56) : 0;
                if (ts[VW_REC + 8 * k + w] + shift != t[VW_REC + 8 * k + w]) bad++;
            }
        // a section one byte too long or too short, a preprocessing section of the wrong size: VW_SECTION / VW_SHORT, never a read outside
        for (int i = 0; i < 4; i++)
            for (int delta = -1; delta <= 1; delta += 2) {
                uint64_t l2[4] = {lens[0], lens[1], lens[2], lens[3]};
                l2[i] += delta;
                uint64_t sum = l2[0] + l2[1] + l2[2] + l2[3];
                std::vector<uint8_t> s2(sec);
                s2.resize(sum, 0);
                if (walk("sections-off", s2.data(), s2.size(), VW_FRAMING_SECTIONS, l2, ts.data()) == VW_OK) bad++;
            }
        if (!prefixes) continue;
        for (size_t n = 0; n < d.size(); n++)
            if (walk("prefix", d.data(), n, VW_FRAMING_PROOF, nullptr, ts.data(), false) != VW_SHORT) bad++;
        printf("prefixes %zu\n", d.size());
        const uint64_t at[4] = {32, t[VW_PRE] - 8, t[VW_PRE] + (uint64_t)VW_N_PRE * 48, t[VW_PRE + 1] - 8};
        const uint64_t counts[4] = {0, 39, 41, 1ull << 63};
        for (int i = 0; i < 4; i++)
            for (uint64_t c : counts) {
                std::vector<uint8_t> m(d);
                for (int b = 0; b < 8; b++) m[at[i] + b] = (uint8_t)(c >> (8 * b));
                if (walk("count", m.data(), m.size(), VW_FRAMING_PROOF, nullptr, ts.data()) != VW_COUNT) bad++;
            }
        prefixes = false;
    }
    printf("bad %d\n", bad);
    return bad ? 1 : 0;
}
