// rv_witness_parse / rv_witness_write (host only, no GPU): the definition of the witness text -- the reference's witness reader scans
// the file byte by byte, '0' and '1' are bits and every other byte is ignored -- that rv_witness_parse_device, rv_witness_reader_* and
// rv_witness_write_device follow.  Which bytes are kept, what they are worth and which bit an output byte shows is witness_text.h's
// to say: the text is walked in the kernels' lanes of 16 bytes.
#include <string.h>

#include "witness_text.h"

namespace {
// the lane at text + at as four words: whole lanes by one copy, the last one byte by byte
inline void lane_words(const uint8_t* text, size_t len, size_t at, uint32_t w[4]) {
    if (len - at >= rv::WT_LANE_BYTES) memcpy(w, text + at, rv::WT_LANE_BYTES);
    else rv::wt_lane_bytes(text + at, text, text + len, w);
}
}  // namespace

extern "C" int rv_witness_parse(const char* text, size_t len, uint8_t* bits, size_t cap, size_t* n_bits) {
    if (!n_bits || (!text && len)) return RV_E_ARG;
    const uint8_t* t = (const uint8_t*)text;
    uint32_t w[4];
    size_t count = 0;
    for (size_t at = 0; at < len; at += rv::WT_LANE_BYTES) {
        lane_words(t, len, at, w);
        count += rv::wt_lane_count(w);
    }
    *n_bits = count;
    if (!bits) return RV_OK;
    if (cap < count) return RV_E_ARG;
    for (size_t at = 0; at < len; at += rv::WT_LANE_BYTES) {
        lane_words(t, len, at, w);
        const uint32_t mask = rv::wt_keep_mask(w);
        if (mask == 0xFFFFu) {  // (a lane of bits alone, the common one: four words at once)
            const uint32_t v[4] = {rv::wt_bit_values(w[0]), rv::wt_bit_values(w[1]), rv::wt_bit_values(w[2]), rv::wt_bit_values(w[3])};
            memcpy(bits, v, sizeof v);
            bits += rv::WT_LANE_BYTES;
            continue;
        }
        rv::wt_lane_values(w, mask, bits);
        bits += __builtin_popcount(mask);
    }
    return RV_OK;
}

extern "C" int rv_witness_write(const uint8_t* bits, size_t n, uint64_t line_bits, char* text, size_t cap, size_t* len) {
    if (!len || (!bits && n)) return RV_E_ARG;
    const uint64_t need = rv::wt_text_len(n, line_bits);
    if (need < n || need > (uint64_t)(size_t)-1) return RV_E_UNSUPPORTED;  // (only where size_t is all of memory)
    *len = (size_t)need;
    if (!text) return RV_OK;
    if (cap < need) return RV_E_ARG;
    return rv::wt_write_range(0, need, rv::wt_line(n, line_bits), n, bits, (uint8_t*)text) ? RV_E_ARG : RV_OK;
}
