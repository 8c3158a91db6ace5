"""An independent numpy model of the linker's rule (include/reverie_amd.h, "programs linked from circuit blocks"), written from the
rule's text and sharing no code with reverie_amd/csrc/link.h.  A netlist is a `Spec`; `check` gives the code and the info, `link` the
whole list, `link_range` any range of ordinals without the whole list.  TEST INFRASTRUCTURE."""
from __future__ import annotations

import numpy as np

from reverie_amd.ops import OP_DTYPE, largest_wires

OK, OOB, BAD, UNSUPPORTED, ARG = 0, 3, 5, 8, 9
WITNESS = 0xFFFFFFFF
EMPTY = np.zeros(0, OP_DTYPE)


def prog(ops):
    return np.array(list(ops), dtype=OP_DTYPE) if not isinstance(ops, np.ndarray) else np.ascontiguousarray(ops)


class Spec:
    """blocks: [(ops, (z64_wires, gf2_wires))]; block_of, bindings: sequences of integers; head, tail: op lists"""

    def __init__(self, blocks=(), block_of=(), bindings=(), head=(), tail=(), z64_base=0, gf2_base=0):
        self.blocks = [(prog(o), (int(w[0]), int(w[1]))) for o, w in blocks]
        self.block_of = np.asarray(list(block_of), dtype=np.uint32)
        self.bindings = np.asarray(list(bindings), dtype=np.uint32)
        self.head, self.tail = prog(head), prog(tail)
        self.z64_base, self.gf2_base = int(z64_base), int(gf2_base)


def is_input(a):
    return (a["domain"] <= 1) & (a["opcode"] == 0)


def _malformed(a):
    return (a["reserved"] != 0) | (a["domain"] > 3) | ((a["domain"] <= 1) & (a["opcode"] > 9))


def _named(a):
    """which of dst, a, b name a wire of the record's own domain (GF(2) and Z64 records)"""
    plain, opc = a["domain"] <= 1, a["opcode"]
    return plain & (opc != 8), plain & ~np.isin(opc, (0, 1, 9)), plain & np.isin(opc, (2, 4, 6))


def _block_code(a, wires):
    """the code of the first record of a block that has one"""
    z, g = wires
    own = np.where(a["domain"] == 0, g, z).astype(np.uint64)
    nd, na, nb = _named(a)
    dst, fa, fb = a["dst"].astype(np.uint64), a["a"].astype(np.uint64), a["b"].astype(np.uint64)
    oob = (nd & (dst >= own)) | (na & (fa >= own)) | (nb & (fb >= own))
    b2a = a["domain"] == 2
    oob |= b2a & ((dst >= z) | (fa + 64 > g))
    code = np.where(_malformed(a), BAD, np.where(a["domain"] == 3, UNSUPPORTED, np.where(oob, OOB, OK)))
    hit = np.flatnonzero(code)
    return int(code[hit[0]]) if len(hit) else OK


def _tables(s: Spec):
    """per instance: op offset, Z, G, B (exclusive, one entry more: the totals), and per block the port count"""
    ports = np.array([int(np.count_nonzero(is_input(o))) for o, _ in s.blocks], dtype=np.uint64)
    n_ops = np.array([len(o) for o, _ in s.blocks], dtype=np.uint64)
    zs = np.array([w[0] for _, w in s.blocks], dtype=np.uint64)
    gs = np.array([w[1] for _, w in s.blocks], dtype=np.uint64)
    bo = s.block_of.astype(np.int64)

    def excl(v):
        return np.concatenate([np.zeros(1, np.uint64), np.cumsum(v[bo], dtype=np.uint64)]) if len(bo) else np.zeros(1, np.uint64)

    return excl(n_ops), excl(zs), excl(gs), excl(ports)


def check(s: Spec):
    """-> (code, info or None), the first code in the rule's order of decisions"""
    for o, w in s.blocks:
        if w[0] > 1 << 32 or w[1] > 1 << 32:
            return ARG, None
    for o, w in s.blocks:
        c = _block_code(o, w)
        if c:
            return c, None
    for end in (s.head, s.tail):
        if _malformed(end).any():
            return BAD, None
    if (s.block_of >= len(s.blocks)).any():
        return ARG, None
    off, Z, G, B = _tables(s)
    if len(s.bindings) != int(B[-1]):
        return ARG, None
    ends = np.concatenate([s.head, s.tail])
    z, g = largest_wires(ends) if len(ends) else (0, 0)
    if len(s.block_of):
        zt, gt = s.z64_base + int(Z[-1]), s.gf2_base + int(G[-1])
        if zt >= 1 << 32 or gt >= 1 << 32:
            return UNSUPPORTED, None
        z, g = max(z, zt), max(g, gt)
    if z > 1 << 32 or g > 1 << 32:
        return UNSUPPORTED, None
    # the bindings in order, with the domain of each one's port
    n_g, n_z = int(np.count_nonzero(is_input(ends) & (ends["domain"] == 0))), int(np.count_nonzero(is_input(ends) & (ends["domain"] == 1)))
    if len(s.bindings):
        doms = [o["domain"][is_input(o)] for o, _ in s.blocks]
        dom = np.concatenate([doms[b] for b in s.block_of.tolist()]) if len(s.block_of) else np.zeros(0, np.uint8)
        bound = s.bindings != WITNESS
        if (bound & (s.bindings.astype(np.uint64) >= np.where(dom == 0, g, z).astype(np.uint64))).any():
            return OOB, None
        n_g += int(np.count_nonzero(~bound & (dom == 0)))
        n_z += int(np.count_nonzero(~bound & (dom == 1)))
    info = dict(n_ops=len(s.head) + int(off[-1]) + len(s.tail), n_instances=len(s.block_of), n_input_gf2=n_g, n_input_z64=n_z, z64_wires=z,
                gf2_wires=g, wire_counts=(z, g))
    return OK, info


def _instances(s: Spec, k, tables):
    """records of the instance region at its ordinals k (uint64 array)"""
    off, Z, G, B = tables
    inst = np.searchsorted(off[:-1], k, side="right") - 1  # the last instance whose offset is <= k: it is not empty
    r = (k - off[inst]).astype(np.int64)
    which = s.block_of[inst]
    out = np.zeros(len(k), OP_DTYPE)
    for b in np.unique(which).tolist():
        sel = np.flatnonzero(which == b)
        ops = s.blocks[b][0]
        rec = ops[r[sel]].copy()
        zb = (s.z64_base + Z[inst[sel]]).astype(np.uint64)
        gb = (s.gf2_base + G[inst[sel]]).astype(np.uint64)
        own = np.where(rec["domain"] == 0, gb, zb)
        nd, na, nb = _named(rec)
        for field, named in (("dst", nd), ("a", na), ("b", nb)):
            rec[field] = np.where(named, rec[field].astype(np.uint64) + own, rec[field]).astype(np.uint32)
        b2a = rec["domain"] == 2
        rec["dst"] = np.where(b2a, rec["dst"].astype(np.uint64) + zb, rec["dst"]).astype(np.uint32)
        rec["a"] = np.where(b2a, rec["a"].astype(np.uint64) + gb, rec["a"]).astype(np.uint32)
        # the ports: Input records in list order; a bound one becomes a copy
        inp = is_input(ops)
        port = (np.cumsum(inp) - inp).astype(np.uint64)
        m = np.flatnonzero(inp[r[sel]])
        if len(m):
            val = s.bindings[(B[inst[sel][m]] + port[r[sel][m]]).astype(np.int64)]
            bound = m[val != WITNESS]
            rec["opcode"][bound] = 3
            rec["a"][bound] = val[val != WITNESS]
            rec["b"][bound] = 0
            rec["imm"][bound] = 0
        out[sel] = rec
    return out


def link_range(s: Spec, first: int, n: int):
    """records first .. first + n - 1 of the output of a netlist that `check` passes, and their Input counts (gf2, z64)"""
    tables = _tables(s)
    n_head, n_inst = len(s.head), int(tables[0][-1])
    j = np.arange(first, first + n, dtype=np.uint64)
    out = np.zeros(n, OP_DTYPE)
    h = j < n_head
    t = j >= n_head + n_inst
    out[h] = s.head[j[h].astype(np.int64)]
    out[t] = s.tail[(j[t] - np.uint64(n_head + n_inst)).astype(np.int64)]
    mid = ~h & ~t
    if mid.any():
        out[mid] = _instances(s, j[mid] - np.uint64(n_head), tables)
    inp = is_input(out)
    return out, (int(np.count_nonzero(inp & (out["domain"] == 0))), int(np.count_nonzero(inp & (out["domain"] == 1))))


def link(s: Spec):
    """-> (code, the whole list or None, info or None)"""
    code, info = check(s)
    if code:
        return code, None, None
    return OK, link_range(s, 0, info["n_ops"])[0], info
