"""Two Python models of the pruning rule (include/reverie_amd.h: rv_ops_prune) that share no code with the library, and
with each other only `shape`, the reading of one record:
  sweep(ops, outs_gf2, outs_z64)  the backward sweep with a needed set per domain -- the definition;
  peel(ops, outs_gf2, outs_z64)   reader counts per value and frontier layers peeled one after the other -- the device's order of
                                  work -- with the number of layers ("device_rounds") and their widths ("widths").
Both return (keep flags, info dict).  `check` is the validation (compile_ops' codes) and the output range rule."""
from __future__ import annotations

import numpy as np

OK, WIRE_OOB, BAD_OP, UNSUPPORTED, ARG = 0, 3, 5, 8, 9
G, Z = 0, 1
CLASSES = ("dropped_gf2_mul", "dropped_z64_mul", "dropped_b2a", "dropped_gf2_random", "dropped_z64_random", "dropped_gf2_other",
           "dropped_z64_other", "unread_gf2_inputs", "unread_z64_inputs")
TWO, ONE = (2, 4, 6), (3, 5, 7, 8)  # opcodes that read a and b / a alone


def shape(rec):
    """rec: a record as a tuple (domain, opcode, reserved, dst, a, b, imm) -> (domain the record defines a value in or None, dst,
    domain of its reads, the indices it reads, root?, drop class)"""
    dom, opc, _, dst, a, b, _ = rec
    if dom == 3:
        return None, 0, G, (), True, None
    if dom == 2:
        return Z, dst, G, tuple(range(a, a + 64)), False, "dropped_b2a"
    d = G if dom == 0 else Z
    reads = (a, b) if opc in TWO else (a,) if opc in ONE else ()
    if opc == 8:
        return None, 0, d, reads, True, None
    cls = "dropped_%s_%s" % ("gf2" if d == G else "z64", "mul" if opc == 6 else "random" if opc == 1 else "other")
    return d, dst, d, reads, opc == 0, cls


def check(ops, wc, outs_gf2=(), outs_z64=()):
    """-> the code: compile_ops' for the first bad op, else ARG for an output index at or above its domain's final count"""
    n = [int(wc[1]), int(wc[0])]
    for rec in ops.tolist():
        dom, opc, reserved, dst, a, b, _ = rec
        if reserved != 0:
            return BAD_OP
        if dom == 3:
            n = [max(n[G], b), max(n[Z], a)]
        elif dom == 2:
            if dst >= n[Z] or a + 64 > n[G]:
                return WIRE_OOB
        elif dom > 3 or opc > 9:
            return BAD_OP
        else:
            d, dst, rd, reads, _, _ = shape(rec)
            if (d is not None and dst >= n[rd]) or any(w >= n[rd] for w in reads):
                return WIRE_OOB
    if any(int(w) >= n[G] for w in outs_gf2) or any(int(w) >= n[Z] for w in outs_z64):
        return ARG
    return OK


def _info(shapes, keep, unread):
    info = {k: 0 for k in CLASSES}
    info["n_kept"] = int(np.count_nonzero(keep))
    info["n_dropped"] = len(keep) - info["n_kept"]
    for i in np.flatnonzero(~keep).tolist():
        info[shapes[i][5]] += 1
    for i in unread:
        info["unread_gf2_inputs" if shapes[i][0] == G else "unread_z64_inputs"] += 1
    return info


def sweep(ops, outs_gf2=(), outs_z64=()):
    shapes = [shape(r) for r in ops.tolist()]
    need = [set(int(w) for w in outs_gf2), set(int(w) for w in outs_z64)]
    keep = np.zeros(len(shapes), bool)
    unread = []
    for i in range(len(shapes) - 1, -1, -1):
        d, dst, rd, reads, root, _ = shapes[i]
        wanted = d is not None and dst in need[d]
        if wanted:
            need[d].discard(dst)
        if not (wanted or root):
            continue
        keep[i] = True
        if d is not None and not wanted:
            unread.append(i)
        need[rd].update(reads)
    info = _info(shapes, keep, unread)
    info["device_rounds"] = info["on_device"] = 0
    return keep, info


def peel(ops, outs_gf2=(), outs_z64=()):
    shapes = [shape(r) for r in ops.tolist()]
    n = len(shapes)
    # every read resolved to the value (the defining op) it reads, forwards; one count per read and per output entry
    cur = [{}, {}]
    reads_of = [[] for _ in range(n)]
    count = [0] * n
    for i, (d, dst, rd, reads, _, _) in enumerate(shapes):
        for w in reads:
            v = cur[rd].get(w)
            if v is not None:
                reads_of[i].append(v)
                count[v] += 1
        if d is not None:
            cur[d][dst] = i
    for d, outs in ((G, outs_gf2), (Z, outs_z64)):
        for w in outs:
            v = cur[d].get(int(w))
            if v is not None:
                count[v] += 1
    keep = np.ones(n, bool)
    frontier = [i for i, s in enumerate(shapes) if s[0] is not None and not s[4] and count[i] == 0]
    widths = []
    while frontier:
        widths.append(len(frontier))
        nxt = []
        for i in frontier:
            keep[i] = False
            for v in reads_of[i]:
                count[v] -= 1
                if count[v] == 0 and not shapes[v][4]:
                    nxt.append(v)
        frontier = nxt
    unread = [i for i, s in enumerate(shapes) if s[0] is not None and s[4] and count[i] == 0]
    info = _info(shapes, keep, unread)
    info["device_rounds"], info["on_device"], info["widths"] = len(widths), 1, widths
    return keep, info
