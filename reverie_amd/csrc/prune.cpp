// rv_ops_prune: the ops no assertion or output depends on, dropped -- the backward sweep (host only; see include/reverie_amd.h and
// DESIGN §23 for the rule).  prune_dev.hip reaches the same kept set by counting readers and peeling; both give the same bytes, and
// both take every per-record decision from prune.h.
//
// One needed flag per index and domain.  The list is walked from the last op to the first: a defining op is kept if its index is
// needed or it is a root, and clears the flag (earlier reads of the index refer to earlier values); a kept op then sets the flags of
// what it reads.  One byte per op for the keep flags, one per wire index for the needed flags (a hash set where the indices are
// sparse, as compact.cpp chooses).
#include <string.h>

#include <algorithm>
#include <unordered_set>
#include <vector>

#include "prune.h"

namespace {
using namespace rv;

// index -> needed
struct Needed {
    std::vector<uint8_t> dense;
    std::unordered_set<uint32_t> sparse;
    bool use_sparse = false;
    void init(uint64_t wires, size_t n_ops) {
        use_sparse = wires > 8 * (uint64_t)n_ops + 65536;
        if (!use_sparse) dense.assign((size_t)wires, 0);
    }
    void set(uint32_t w) {
        if (use_sparse) sparse.insert(w);
        else dense[w] = 1;
    }
    // the flag, cleared
    bool take(uint32_t w) {
        if (use_sparse) return sparse.erase(w) != 0;
        const bool was = dense[w] != 0;
        dense[w] = 0;
        return was;
    }
};

// The three passes over the windows [0, cuts[0]), [cuts[0], cuts[1]), .. [cuts[n_cuts - 1], n): the validation forwards (the counts in
// force run on from window to window), the window step (prune.h: pr_window_sweep) from the last window to the first with the needed
// tables handed on, the kept records forwards.  rv_ops_prune is this with no cut.
int sweep(const rv_op* ops, size_t n, size_t z64_wires, size_t gf2_wires, const uint32_t* outs[2], const size_t n_outs[2], const size_t* cuts,
          size_t n_cuts, rv_op* out, size_t cap, size_t* n_out, uint32_t* old_index, rv_prune_info* info) {
    if (n >= PR_NONE - 1) return RV_E_UNSUPPORTED;
    for (size_t c = 0; c < n_cuts; c++)
        if (cuts[c] > n || (c && cuts[c] < cuts[c - 1])) return RV_E_ARG;
    uint64_t nw[2] = {gf2_wires, z64_wires};
    for (size_t i = 0; i < n; i++) {
        if (ops[i].domain == RV_DOM_SIZEHINT && ops[i].reserved == 0)
            nw[PR_G] = std::max<uint64_t>(nw[PR_G], ops[i].b), nw[PR_Z] = std::max<uint64_t>(nw[PR_Z], ops[i].a);
        if (const int rc = pr_check(ops[i], nw[PR_Z], nw[PR_G])) return rc;
    }
    for (int d = 0; d < 2; d++)
        for (size_t k = 0; k < n_outs[d]; k++)
            if (outs[d][k] >= nw[d]) return RV_E_ARG;

    Needed need[2];
    need[PR_G].init(nw[PR_G], n), need[PR_Z].init(nw[PR_Z], n);
    for (int d = 0; d < 2; d++)
        for (size_t k = 0; k < n_outs[d]; k++) need[d].set(outs[d][k]);
    std::vector<uint8_t> keep(n);
    rv_prune_info pi = {};
    uint64_t* cls = &pi.dropped_gf2_mul;  // (the nine class counters lie in prune.h's order)
    // the windows from the last to the first (no cut: the whole list is the one window)
    for (size_t c = n_cuts + 1; c-- > 0;) {
        const size_t lo = c ? cuts[c - 1] : 0, hi = c < n_cuts ? cuts[c] : n;
        pi.n_kept += pr_window_sweep(ops + lo, hi - lo, need, keep.data() + lo, cls);
    }
    pi.n_dropped = n - pi.n_kept;

    // (every allocation is made by here: nothing below fails, so `out` is written whole or not at all)
    if (out) {
        if (cap < pi.n_kept) return RV_E_ARG;
        size_t at = 0;
        for (size_t i = 0; i < n; i++) {
            if (!keep[i]) continue;
            if (out + at != ops + i) memmove(out + at, ops + i, sizeof(rv_op));  // (in place: at <= i)
            if (old_index) old_index[at] = (uint32_t)i;
            at++;
        }
    }
    if (n_out) *n_out = (size_t)pi.n_kept;
    if (info) *info = pi;
    return RV_OK;
}

}  // namespace

extern "C" int rv_ops_prune_windows_host(const rv_op* ops, size_t n_ops, size_t z64_wires, size_t gf2_wires, const uint32_t* outputs_gf2,
                                         size_t n_outputs_gf2, const uint32_t* outputs_z64, size_t n_outputs_z64, const size_t* cuts, size_t n_cuts,
                                         rv_op* out, size_t cap, size_t* n_out, uint32_t* old_index, rv_prune_info* info) {
    if ((n_ops && !ops) || (n_outputs_gf2 && !outputs_gf2) || (n_outputs_z64 && !outputs_z64) || (n_cuts && !cuts)) return RV_E_ARG;
    // (out == ops is the in-place form; any other overlap would have the copy read what it wrote)
    if (n_ops && out && out != ops && (const uint8_t*)out < (const uint8_t*)(ops + n_ops) && (const uint8_t*)ops < (const uint8_t*)(out + cap))
        return RV_E_ARG;
    const uint32_t* outs[2] = {outputs_gf2, outputs_z64};
    const size_t n_outs[2] = {n_outputs_gf2, n_outputs_z64};
    try {  // no C++ exception may cross the C boundary
        return sweep(ops, n_ops, z64_wires, gf2_wires, outs, n_outs, cuts, n_cuts, out, cap, n_out, old_index, info);
    } catch (...) {
        return RV_E_NOMEM;
    }
}

extern "C" int rv_ops_prune(const rv_op* ops, size_t n_ops, size_t z64_wires, size_t gf2_wires, const uint32_t* outputs_gf2, size_t n_outputs_gf2,
                            const uint32_t* outputs_z64, size_t n_outputs_z64, rv_op* out, size_t cap, size_t* n_out, uint32_t* old_index,
                            rv_prune_info* info) {
    return rv_ops_prune_windows_host(ops, n_ops, z64_wires, gf2_wires, outputs_gf2, n_outputs_gf2, outputs_z64, n_outputs_z64, nullptr, 0, out, cap, n_out,
                                     old_index, info);
}
