// rv_link: a program linked from circuit blocks, the sequential definition (host only; see include/reverie_amd.h and DESIGN §22 for
// the rule).  link_dev.hip is the same rule in parallel form; both give the same bytes, and both take every per-record decision
// from link.h.
//
// One pass over the blocks (judge, count the ports), one over the instances (sums, block_of), one over the bindings, then the
// output is written instance by instance.  Beside the output: 8 bytes per block.
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "link.h"

using namespace rv;

extern "C" int rv_link(const rv_link_desc* d, rv_op** ops, rv_link_info* info) {
    if (ops) *ops = nullptr;
    if (!info) return RV_E_ARG;
    try {
        // (1) arguments
        uint64_t block_ops = 0;
        if (const int rc = lk_check_args(d, &block_ops)) return rc;
        // (2) blocks in order
        std::vector<uint64_t> ports(d->n_blocks);
        for (uint64_t b = 0; b < d->n_blocks; b++) {
            const rv_link_block& k = d->blocks[b];
            const uint64_t* w = reinterpret_cast<const uint64_t*>(k.ops);
            for (uint64_t r = 0; r < k.n_ops; r++, w += 3) {
                if (const int c = lk_judge(w, k.z64_wires, k.gf2_wires)) return c;
                ports[b] += lk_is_input(w[0]);
            }
        }
        // (3) head, (4) tail
        LkEnds ends;
        if (const int c = lk_judge_end(d->head, d->n_head, ends)) return c;
        if (const int c = lk_judge_end(d->tail, d->n_tail, ends)) return c;
        // (5) instances in order, the binding count, the wire counts
        uint64_t inst_ops = 0, z_sum = 0, g_sum = 0, n_ports = 0;
        for (uint64_t i = 0; i < d->n_instances; i++) {
            const uint32_t b = d->block_of[i];
            if (b >= d->n_blocks) return RV_E_ARG;
            inst_ops += d->blocks[b].n_ops, z_sum += d->blocks[b].z64_wires, g_sum += d->blocks[b].gf2_wires, n_ports += ports[b];
        }
        if (d->n_bindings != n_ports) return RV_E_ARG;
        rv_link_info res = {};
        if (const int c = lk_wire_counts(d, ends, z_sum, g_sum, &res.z64_wires, &res.gf2_wires)) return c;
        // (6) bindings in order
        res.n_ops = d->n_head + inst_ops + d->n_tail, res.n_instances = d->n_instances;
        res.n_input_gf2 = ends.in_gf2, res.n_input_z64 = ends.in_z64;
        const uint32_t* bind = d->bindings;
        for (uint64_t i = 0; i < d->n_instances; i++) {
            const rv_link_block& k = d->blocks[d->block_of[i]];
            const uint64_t* w = reinterpret_cast<const uint64_t*>(k.ops);
            for (uint64_t r = 0; r < k.n_ops; r++, w += 3) {
                if (!lk_is_input(w[0])) continue;
                const bool gf2 = lk_dom(w[0]) == RV_DOM_GF2;
                const uint32_t v = *bind++;
                if (v == RV_LINK_WITNESS) (gf2 ? res.n_input_gf2 : res.n_input_z64)++;
                else if (v >= (gf2 ? res.gf2_wires : res.z64_wires)) return RV_E_WIRE_OOB;
            }
        }
        if (ops) {
            if (res.n_ops > (size_t)-1 / sizeof(rv_op)) return RV_E_NOMEM;
            uint64_t* out = (uint64_t*)malloc(res.n_ops ? (size_t)res.n_ops * sizeof(rv_op) : 1);
            if (!out) return RV_E_NOMEM;
            uint64_t* o = out;
            if (d->n_head) memcpy(o, d->head, (size_t)d->n_head * sizeof(rv_op)), o += 3 * d->n_head;
            uint64_t z = d->z64_base, g = d->gf2_base;
            bind = d->bindings;
            for (uint64_t i = 0; i < d->n_instances; i++) {
                const rv_link_block& k = d->blocks[d->block_of[i]];
                const uint64_t* w = reinterpret_cast<const uint64_t*>(k.ops);
                for (uint64_t r = 0; r < k.n_ops; r++, w += 3, o += 3) lk_rewrite(w, (uint32_t)z, (uint32_t)g, lk_is_input(w[0]) ? *bind++ : 0, o);
                z += k.z64_wires, g += k.gf2_wires;
            }
            if (d->n_tail) memcpy(o, d->tail, (size_t)d->n_tail * sizeof(rv_op));
            *ops = (rv_op*)out;
        }
        *info = res;
        return RV_OK;
    } catch (...) {
        return RV_E_NOMEM;
    }
}
