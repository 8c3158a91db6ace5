// rv_ops_fold, rv_ops_fold_windows_host: constants folded, record for record -- the forward sweep (host only; see
// include/reverie_amd.h and DESIGN §24 for the rule; the sweep itself is fold.h's fd_window_sweep).  fold_dev.hip reaches the same
// known set by propagating from the records that are known at once; both give the same bytes, and both take every per-record
// decision from fold.h.
//
// One known flag and one value per index and domain.  The list is walked from the first op to the last: a record's reads are looked
// up, the record is judged and rewritten (fold.h), and a defining op then sets the flag and the value of its index.  An index no op
// has written yet is known 0.  Nine bytes per wire index (a hash map where the indices are sparse, as prune.cpp chooses).
#include <string.h>

#include <algorithm>
#include <unordered_map>
#include <vector>

#include "fold.h"

namespace {
using namespace rv;

// index -> (known, value): what the sweep carries from op to op (and, for a list cut in windows, from window to window)
struct Known {
    std::vector<uint8_t> flag;
    std::vector<uint64_t> val;
    std::unordered_map<uint32_t, std::pair<bool, uint64_t>> sparse;
    bool use_sparse = false;
    void init(uint64_t wires, size_t n_ops) {
        use_sparse = wires > 8 * (uint64_t)n_ops + 65536;
        if (!use_sparse) flag.assign((size_t)wires, 1), val.assign((size_t)wires, 0);  // nothing written: the zero wire
    }
    bool get(uint32_t w, uint64_t* v) const {
        if (use_sparse) {
            const auto it = sparse.find(w);
            *v = it == sparse.end() ? 0 : it->second.second;
            return it == sparse.end() || it->second.first;
        }
        *v = val[w];
        return flag[w] != 0;
    }
    void set(uint32_t w, bool known, uint64_t v) {
        if (use_sparse) sparse[w] = {known, known ? v : 0};
        else flag[w] = known, val[w] = known ? v : 0;
    }
};

// every record against the counts in force at it; nw: the counts as declared, then as they stand behind the list
int validate(const rv_op* ops, size_t n, uint64_t nw[2]) {
    for (size_t i = 0; i < n; i++) {
        if (ops[i].domain == RV_DOM_SIZEHINT && ops[i].reserved == 0)
            nw[PR_G] = std::max<uint64_t>(nw[PR_G], ops[i].b), nw[PR_Z] = std::max<uint64_t>(nw[PR_Z], ops[i].a);
        if (const int rc = pr_check(ops[i], nw[PR_Z], nw[PR_G])) return rc;
    }
    return RV_OK;
}

// the sweep over the windows [0, cuts[0]), .. [cuts[n_cuts - 1], n) with ONE state (sized by the final counts: an index a later
// SizeHint brings in is known 0 until something writes it, whenever its entry is made)
int fold(const rv_op* ops, size_t n, size_t z64_wires, size_t gf2_wires, const size_t* cuts, size_t n_cuts, rv_op* out, rv_fold_info* info) {
    if (n >= PR_NONE - 1) return RV_E_UNSUPPORTED;
    uint64_t nw[2] = {gf2_wires, z64_wires};
    if (const int rc = validate(ops, n, nw)) return rc;
    Known st[2];
    st[PR_G].init(nw[PR_G], n), st[PR_Z].init(nw[PR_Z], n);
    // (every allocation of the dense form is made by here: `out` is written whole or not at all)
    rv_fold_info fi = {};
    uint64_t* cls = &fi.gf2_mul_to_const;  // (the nine class counters lie in fold.h's order)
    // (a hash map can fail half-way: the records are made beside the list and copied at the end)
    const bool beside = st[PR_G].use_sparse || st[PR_Z].use_sparse;
    std::vector<rv_op> tmp(out && beside ? n : 0);
    rv_op* to = !out ? nullptr : beside ? tmp.data() : out;
    size_t lo = 0;
    for (size_t k = 0; k <= n_cuts; k++) {
        const size_t hi = k < n_cuts ? cuts[k] : n;
        fd_window_sweep(ops + lo, hi - lo, st, to ? to + lo : nullptr, cls, &fi.n_known);
        lo = hi;
    }
    if (out && beside && n) memcpy(out, tmp.data(), n * sizeof(rv_op));
    fi.n_ops = n;
    for (int c = 0; c < FD_REWRITTEN; c++) fi.n_rewritten += cls[c];
    if (info) *info = fi;
    return RV_OK;
}

int fold_checked(const rv_op* ops, size_t n_ops, size_t z64_wires, size_t gf2_wires, const size_t* cuts, size_t n_cuts, rv_op* out, rv_fold_info* info) {
    if (n_ops && !ops) return RV_E_ARG;
    if (n_ops > (size_t)-1 / sizeof(rv_op)) return RV_E_UNSUPPORTED;
    // (out == ops is the in-place form: record j is written from record j; any other overlap would read what was written)
    if (n_ops && out && out != ops && (const uint8_t*)out < (const uint8_t*)(ops + n_ops) && (const uint8_t*)ops < (const uint8_t*)(out + n_ops))
        return RV_E_ARG;
    try {  // no C++ exception may cross the C boundary
        return fold(ops, n_ops, z64_wires, gf2_wires, cuts, n_cuts, out, info);
    } catch (...) {
        return RV_E_NOMEM;
    }
}

}  // namespace

extern "C" int rv_ops_fold(const rv_op* ops, size_t n_ops, size_t z64_wires, size_t gf2_wires, rv_op* out, rv_fold_info* info) {
    return fold_checked(ops, n_ops, z64_wires, gf2_wires, nullptr, 0, out, info);
}

extern "C" int rv_ops_fold_windows_host(const rv_op* ops, size_t n_ops, size_t z64_wires, size_t gf2_wires, const size_t* cuts, size_t n_cuts, rv_op* out,
                                        rv_fold_info* info) {
    if (n_cuts && !cuts) return RV_E_ARG;
    for (size_t k = 0; k < n_cuts; k++)
        if (cuts[k] > n_ops || (k && cuts[k] < cuts[k - 1])) return RV_E_ARG;
    return fold_checked(ops, n_ops, z64_wires, gf2_wires, cuts, n_cuts, out, info);
}

// the fall-back of one windowed device feed (fold_win.hip): the sweep over the feed with the tables as the device holds them
namespace rv {
void fold_window_dense(const rv_op* ops, size_t n, uint8_t* const K[2], uint64_t* const V[2], rv_op* out, uint64_t* cls, uint64_t* n_known) {
    FdDense st[2] = {{K[PR_G], V[PR_G]}, {K[PR_Z], V[PR_Z]}};
    fd_window_sweep(ops, n, st, out, cls, n_known);
}
}  // namespace rv
