// rv_ops_compact_wires: wire indices renumbered by liveness, the sequential sweep (host only; see include/reverie_amd.h and
// DESIGN §17 for the rule).  compact_dev.hip is the same rule in parallel form; both give the same bytes.
//
// Two passes over the list.  Pass 1 resolves every operand to the value it reads (the op that defined it, the zero wire, or a pinned
// index) and records each value's last reader.  Pass 2 is the pool: one FIFO of free slots per domain, the destination allocated
// before the operands are released.  20 bytes per op beside the lists, 4 per wire index (a hash map where the indices are sparse).
#include <string.h>

#include <algorithm>
#include <unordered_map>
#include <vector>

#include "../../include/reverie_amd.h"

namespace {

constexpr uint32_t NONE = 0xFFFFFFFFu;  // an operand that reads the zero wire; a value without a reader
constexpr uint32_t PIN = 0xFFFFFFFEu;   // an operand on a pinned index
constexpr int G = 0, Z = 1;

inline int op_reads(uint8_t opcode) {
    switch (opcode) {
    case RV_OP_ADD: case RV_OP_SUB: case RV_OP_MUL: return 2;
    case RV_OP_ADDCONST: case RV_OP_SUBCONST: case RV_OP_MULCONST: case RV_OP_ASSERTZERO: return 1;
    default: return 0;
    }
}

// compile_ops' checks of one op against the counts in force (nw[G], nw[Z]); a SizeHint raises them
inline int check_op(const rv_op& op, uint64_t nw[2]) {
    if (op.reserved != 0) return RV_E_BAD_OP;
    switch (op.domain) {
    case RV_DOM_SIZEHINT:
        nw[G] = std::max<uint64_t>(nw[G], op.b), nw[Z] = std::max<uint64_t>(nw[Z], op.a);
        return RV_OK;
    case RV_DOM_GF2:
    case RV_DOM_Z64: {
        if (op.opcode > RV_OP_CONST) return RV_E_BAD_OP;
        const uint64_t n = nw[op.domain == RV_DOM_GF2 ? G : Z];
        const int r = op_reads(op.opcode);
        if ((op.opcode != RV_OP_ASSERTZERO && op.dst >= n) || (r >= 1 && op.a >= n) || (r >= 2 && op.b >= n)) return RV_E_WIRE_OOB;
        return RV_OK;
    }
    case RV_DOM_B2A:
        return (op.dst >= nw[Z] || (uint64_t)op.a + 64 > nw[G]) ? RV_E_WIRE_OOB : RV_OK;
    default:
        return RV_E_BAD_OP;
    }
}

// index -> the op that defined the value it holds (NONE: never written)
struct Holders {
    std::vector<uint32_t> dense;
    std::unordered_map<uint32_t, uint32_t> sparse;
    bool use_sparse = false;
    void init(uint64_t wires, size_t n_ops) {
        use_sparse = wires > 8 * (uint64_t)n_ops + 65536;
        if (!use_sparse) dense.assign((size_t)wires, NONE);
    }
    uint32_t get(uint32_t w) const {
        if (!use_sparse) return dense[w];
        const auto it = sparse.find(w);
        return it == sparse.end() ? NONE : it->second;
    }
    void set(uint32_t w, uint32_t i) {
        if (use_sparse) sparse[w] = i;
        else dense[w] = i;
    }
};

// the pinned indices: the union of the B2A ranges as disjoint intervals, each with the rank of its first index
struct Pins {
    std::vector<uint32_t> lo, hi, rank0;  // [lo, hi)
    uint64_t total = 0;
    void build(std::vector<uint32_t>& starts) {
        std::sort(starts.begin(), starts.end());
        for (uint32_t s : starts) {
            if (!lo.empty() && s <= hi.back()) {
                total += (uint64_t)s + 64 - hi.back();
                hi.back() = s + 64;
            } else {
                lo.push_back(s), hi.push_back(s + 64), rank0.push_back((uint32_t)total);
                total += 64;
            }
        }
    }
    bool find(uint32_t w, uint32_t* rank) const {
        if (lo.empty()) return false;
        const size_t k = (size_t)(std::upper_bound(lo.begin(), lo.end(), w) - lo.begin());
        if (k == 0 || w >= hi[k - 1]) return false;
        *rank = rank0[k - 1] + (w - lo[k - 1]);
        return true;
    }
};

int sweep(const rv_op* ops, size_t n, size_t z64_wires, size_t gf2_wires, rv_op* out, rv_compact_info* info) {
    if (n >= NONE - 1) return RV_E_UNSUPPORTED;
    uint64_t nw[2] = {gf2_wires, z64_wires};
    std::vector<uint32_t> starts;
    for (size_t i = 0; i < n; i++) {
        if (const int rc = check_op(ops[i], nw)) return rc;
        if (ops[i].domain == RV_DOM_B2A) starts.push_back(ops[i].a);
    }
    Pins pins;
    pins.build(starts);
    const uint32_t P = (uint32_t)pins.total;

    // pass 1
    Holders cur[2];
    cur[G].init(nw[G], n), cur[Z].init(nw[Z], n);
    std::vector<uint32_t> va(n, NONE), vb(n, NONE), last(n, NONE), slot(n, NONE);
    uint32_t zero[2] = {0, 0};
    uint64_t values[2] = {0, 0}, pool_values[2] = {0, 0};
    for (size_t i = 0; i < n; i++) {
        const rv_op& op = ops[i];
        if (op.domain == RV_DOM_B2A) {
            values[Z]++, pool_values[Z]++;
            cur[Z].set(op.dst, (uint32_t)i);
            continue;
        }
        if (op.domain > RV_DOM_Z64) continue;
        const int d = op.domain == RV_DOM_GF2 ? G : Z;
        const int r = op_reads(op.opcode);
        uint32_t rank;
        for (int k = 0; k < r; k++) {
            const uint32_t w = k ? op.b : op.a;
            uint32_t v;
            if (d == G && pins.find(w, &rank)) {
                v = PIN;
            } else if ((v = cur[d].get(w)) == NONE) {
                zero[d] = 1;
            } else {
                last[v] = (uint32_t)i;
            }
            (k ? vb : va)[i] = v;
        }
        if (op.opcode != RV_OP_ASSERTZERO) {
            values[d]++;
            if (!(d == G && pins.find(op.dst, &rank))) cur[d].set(op.dst, (uint32_t)i), pool_values[d]++;
        }
    }

    // pass 2 (every allocation is made by here: nothing below fails, so `out` is written whole or not at all)
    const uint32_t base[2] = {P + zero[G], zero[Z]};
    uint32_t fresh[2] = {0, 0};
    std::vector<uint32_t> fifo[2];
    size_t head[2] = {0, 0};
    fifo[G].reserve((size_t)pool_values[G]), fifo[Z].reserve((size_t)pool_values[Z]);
    for (size_t i = 0; i < n; i++) {
        rv_op op = ops[i];
        if (op.domain == RV_DOM_SIZEHINT) continue;  // (its fields are the final counts: written below)
        const bool b2a = op.domain == RV_DOM_B2A;
        const int d = (b2a || op.domain == RV_DOM_Z64) ? Z : G;
        const int r = b2a ? 0 : op_reads(op.opcode);
        uint32_t rank = 0;
        const bool defines = b2a || op.opcode != RV_OP_ASSERTZERO;
        const bool pinned_dst = defines && d == G && pins.find(op.dst, &rank);
        if (pinned_dst) {
            op.dst = rank;
        } else if (defines) {
            if (head[d] < fifo[d].size()) slot[i] = fifo[d][head[d]++];
            else slot[i] = base[d] + fresh[d]++;
            op.dst = slot[i];
        }
        if (b2a) {
            pins.find(op.a, &rank);
            op.a = rank;
        }
        for (int k = 0; k < r; k++) {
            const uint32_t v = k ? vb[i] : va[i];
            uint32_t& field = k ? op.b : op.a;
            if (v == PIN) {
                pins.find(field, &rank);
                field = rank;
            } else if (v == NONE) {
                field = d == G ? P : 0;
            } else {
                field = slot[v];
                if (last[v] == i && !(k == 1 && va[i] == v)) fifo[d].push_back(slot[v]);
            }
        }
        if (defines && !pinned_dst && last[i] == NONE) fifo[d].push_back(slot[i]);
        out[i] = op;
    }
    const uint64_t new_z = (uint64_t)zero[Z] + fresh[Z], new_g = (uint64_t)P + zero[G] + fresh[G];
    for (size_t i = 0; i < n; i++)
        if (ops[i].domain == RV_DOM_SIZEHINT) {
            rv_op op = ops[i];
            op.a = (uint32_t)new_z, op.b = (uint32_t)new_g;
            out[i] = op;
        }
    if (info) {
        memset(info, 0, sizeof *info);
        info->z64_wires = new_z, info->gf2_wires = new_g, info->gf2_pinned = P;
        info->gf2_zero_wire = zero[G], info->z64_zero_wire = zero[Z];
        info->gf2_values = values[G], info->z64_values = values[Z];
    }
    return RV_OK;
}

}  // namespace

extern "C" int rv_ops_compact_wires(const rv_op* ops, size_t n_ops, size_t z64_wires, size_t gf2_wires, rv_op* out, rv_compact_info* info) {
    if (n_ops && (!ops || !out)) return RV_E_ARG;
    // (out == ops is the in-place form; any other overlap would have the sweep read what it wrote)
    if (n_ops && out != ops && (const uint8_t*)out < (const uint8_t*)(ops + n_ops) && (const uint8_t*)ops < (const uint8_t*)(out + n_ops)) return RV_E_ARG;
    try {  // no C++ exception may cross the C boundary
        return sweep(ops, n_ops, z64_wires, gf2_wires, out, info);
    } catch (...) {
        return RV_E_NOMEM;
    }
}
