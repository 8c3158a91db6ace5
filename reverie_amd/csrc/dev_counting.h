// The work memory of one call, counted: a DevAlloc in front of another one that remembers how many bytes are out and the most that
// ever were (the windowed stages report it as peak_feed_bytes: win_stage.h's stage_counted, for compact_win.hip, prune_win.hip
// and fold_win.hip).
#pragma once
#include <stddef.h>

#include <algorithm>
#include <unordered_map>

#include "compile_dev.h"

namespace rv {

struct Counting {
    DevAlloc inner;
    size_t cur = 0, peak = 0;
    std::unordered_map<void*, size_t> sizes;
};
inline int counting_alloc(void* self, size_t bytes, void** out) {
    Counting* c = (Counting*)self;
    const int rc = c->inner.alloc(c->inner.self, bytes, out);
    if (rc == RV_OK) {
        c->sizes[*out] = bytes;
        c->cur += bytes;
        c->peak = std::max(c->peak, c->cur);
    }
    return rc;
}
inline void counting_release(void* self, void* p) {
    Counting* c = (Counting*)self;
    const auto it = c->sizes.find(p);
    if (it != c->sizes.end()) c->cur -= it->second, c->sizes.erase(it);
    c->inner.release(c->inner.self, p);
}
// fn(CA) with CA counting in front of A -> fn's code; *peak = the most that was out at once
template <class Fn>
int counted_call(const DevAlloc& A, size_t* peak, Fn&& fn) {
    Counting cnt;
    cnt.inner = A;
    DevAlloc CA;
    CA.self = &cnt, CA.alloc = counting_alloc, CA.release = counting_release;
    const int rc = fn(CA);
    *peak = cnt.peak;
    return rc;
}

}  // namespace rv
