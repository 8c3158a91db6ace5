"""A Python model of the folding rule (include/reverie_amd.h: rv_ops_fold) that shares no code with the library: plain
dicts per wire index.
  fold(ops)    the forward sweep -- the definition -> (folded records, info dict, kinds): kinds[j] names what became of record j
               (one of KINDS, or None where it stayed);
  layers(ops)  the device's order of work: the records known at once are layer 0, and a record is in layer r + 1 when something in
               layer r made it known -> (the layer of every known record as a dict, the widths of the layers).
  check(ops, wc)  the validation (compile_ops' codes)."""
from __future__ import annotations

import numpy as np

OK, WIRE_OOB, BAD_OP, UNSUPPORTED, ARG = 0, 3, 5, 8, 9
M64 = (1 << 64) - 1
INPUT, RANDOM, ADD, ADDC, SUB, SUBC, MUL, MULC, ASSERT, CONST = range(10)
COUNTS = ("gf2_mul_to_const", "z64_mul_to_const", "gf2_mul_to_linear", "z64_mul_to_linear", "b2a_to_const", "gf2_other_rewritten",
          "z64_other_rewritten", "asserts_known_zero", "asserts_known_nonzero")
# what a record became, by domain ("g" / "z") where it matters; the two "left" kinds are records with a known read that stay
KINDS = ("g_mul_const", "z_mul_const", "g_mul_linear", "z_mul_linear", "b2a_const", "g_add_addconst", "z_add_addconst", "g_sub_subconst",
         "z_sub_subconst", "g_sub_addconst", "g_linear_const", "z_linear_const", "g_zero_mulconst", "z_zero_mulconst", "left_z_sub_a_known",
         "left_b2a_unknown_bit")


def check(ops, wc):
    n = {0: int(wc[1]), 1: int(wc[0])}
    for dom, opc, reserved, dst, a, b, _ in ops.tolist():
        if reserved != 0:
            return BAD_OP
        if dom == 3:
            n = {0: max(n[0], b), 1: max(n[1], a)}
        elif dom == 2:
            if dst >= n[1] or a + 64 > n[0]:
                return WIRE_OOB
        elif dom > 3 or opc > 9:
            return BAD_OP
        else:
            used = [dst] if opc != ASSERT else []
            used += [a] if opc in (ADD, ADDC, SUB, SUBC, MUL, MULC, ASSERT) else []
            used += [b] if opc in (ADD, SUB, MUL) else []
            if any(w >= n[dom] for w in used):
                return WIRE_OOB
    return OK


def _value(dom, opc, x, y, c):
    """the evaluator's arithmetic: GF(2) one bit, Z64 wrapping"""
    if dom == 0:
        return {ADD: x ^ y, SUB: x ^ y, MUL: x & y, ADDC: x ^ c, SUBC: x ^ c, MULC: x & c}[opc]
    return {ADD: x + y, SUB: x - y, MUL: x * y, ADDC: x + c, SUBC: x - c, MULC: x * c}[opc] & M64


def fold(ops):
    known = [{}, {}]  # index -> value, where the value now on the index is known
    written = [set(), set()]
    out = ops.copy()
    info = {k: 0 for k in ("n_ops", "n_rewritten", "n_known") + COUNTS + ("device_rounds", "on_device")}
    info["n_ops"] = len(ops)
    kinds = [None] * len(ops)

    def read(d, w):
        """-> the value, or None where it is not known (an index nobody wrote is the zero wire)"""
        return known[d].get(w) if w in written[d] else 0

    def put(j, d, dst, v, kind, count):
        known[d][dst] = v
        written[d].add(dst)
        info["n_known"] += 1
        if kind is not None:
            out[j] = (d, CONST, 0, dst, 0, 0, v)
            kinds[j] = kind
            info[count] += 1

    def unknown(d, dst):
        known[d].pop(dst, None)
        written[d].add(dst)

    for j, (dom, opc, _, dst, a, b, imm) in enumerate(ops.tolist()):
        if dom == 3:
            continue
        if dom == 2:
            bits = [read(0, a + k) for k in range(64)]
            if all(v is not None for v in bits):
                put(j, 1, dst, sum(v << k for k, v in enumerate(bits)), "b2a_const", "b2a_to_const")
            else:
                unknown(1, dst)
                if any(v is not None for v in bits):
                    kinds[j] = "left_b2a_unknown_bit"
            continue
        t = "gz"[dom]
        other = ("gf2" if dom == 0 else "z64") + "_other_rewritten"
        c = imm & 1 if dom == 0 else imm
        if opc == ASSERT:
            x = read(dom, a)
            if x is not None:
                info["asserts_known_zero" if x == 0 else "asserts_known_nonzero"] += 1
        elif opc in (INPUT, RANDOM):
            unknown(dom, dst)
        elif opc == CONST:
            put(j, dom, dst, c, None, None)
        elif opc in (ADDC, SUBC, MULC):
            x = read(dom, a)
            if opc == MULC and c == 0:
                put(j, dom, dst, 0, t + "_zero_mulconst" if x is None else t + "_linear_const", other)
            elif x is not None:
                put(j, dom, dst, _value(dom, opc, x, 0, c), t + "_linear_const", other)
            else:
                unknown(dom, dst)
        else:
            x, y = read(dom, a), read(dom, b)
            if x is not None and y is not None:
                v = _value(dom, opc, x, y, 0)
                if opc == MUL:
                    put(j, dom, dst, v, t + "_mul_const", ("gf2" if dom == 0 else "z64") + "_mul_to_const")
                else:
                    put(j, dom, dst, v, t + "_linear_const", other)
            elif opc == MUL and (x == 0 or y == 0):
                put(j, dom, dst, 0, t + "_mul_const", ("gf2" if dom == 0 else "z64") + "_mul_to_const")
            else:
                unknown(dom, dst)
                if x is None and y is None:
                    continue
                if opc == MUL:
                    out[j] = (dom, MULC, 0, dst, b if y is None else a, 0, x if y is None else y)
                    kinds[j] = t + "_mul_linear"
                    info[("gf2" if dom == 0 else "z64") + "_mul_to_linear"] += 1
                elif opc == ADD:
                    out[j] = (dom, ADDC, 0, dst, b if y is None else a, 0, x if y is None else y)
                    kinds[j] = t + "_add_addconst"
                    info[other] += 1
                elif y is not None:
                    out[j] = (dom, SUBC, 0, dst, a, 0, y)
                    kinds[j] = t + "_sub_subconst"
                    info[other] += 1
                elif dom == 0:
                    out[j] = (dom, ADDC, 0, dst, b, 0, x)
                    kinds[j] = "g_sub_addconst"
                    info[other] += 1
                else:
                    kinds[j] = "left_z_sub_a_known"
    info["n_rewritten"] = sum(info[k] for k in COUNTS[:7])
    return out, info, kinds


def layers(ops):
    """-> ({op: layer} for the known records, the layers' widths).  The values are fold()'s; this gives the order they are found in."""
    cur = [{}, {}]  # index -> the op whose value is on it
    layer, value = {}, {}
    for j, (dom, opc, _, dst, a, b, imm) in enumerate(ops.tolist()):
        if dom == 3:
            continue
        rd = 0 if dom in (0, 2) else 1
        reads = [a + k for k in range(64)] if dom == 2 else [a, b] if opc in (ADD, SUB, MUL) else [a] if opc in (ADDC, SUBC, MULC, ASSERT) else []
        prods = [cur[rd].get(w) for w in reads]
        d = 1 if dom == 2 else dom
        if dom != 2 and opc == ASSERT:
            continue
        cur[d][dst] = j
        if dom != 2 and opc in (INPUT, RANDOM):
            continue
        c = imm & 1 if dom == 0 else imm
        if (dom != 2 and (opc == CONST or (opc == MULC and c == 0))) or all(p is None for p in prods) or (dom != 2 and opc == MUL and None in prods):
            layer[j] = 0  # known at once
        else:
            at = [layer.get(p) for p in prods if p is not None]
            by_all = None if any(x is None for x in at) else max(at) + 1
            zeros = [layer[p] + 1 for p in prods if p is not None and p in layer and value[p] == 0] if dom != 2 and opc == MUL else []
            found = [x for x in zeros + [by_all] if x is not None]
            if not found:
                continue
            layer[j] = min(found)
        vals = [0 if p is None else value.get(p, 0) for p in prods]
        if dom == 2:
            value[j] = sum((v & 1) << k for k, v in enumerate(vals))
        elif opc == CONST:
            value[j] = c
        elif opc == MULC and c == 0:
            value[j] = 0
        elif opc == MUL and any(p is None or (p in layer and value[p] == 0) for p in prods):
            value[j] = 0
        else:
            value[j] = _value(dom, opc, vals[0], vals[1] if len(vals) > 1 else 0, c)
    widths = [0] * (max(layer.values()) + 1 if layer else 0)
    for r in layer.values():
        widths[r] += 1
    return layer, widths
