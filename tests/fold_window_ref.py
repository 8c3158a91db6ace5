"""A Python model of the folding WINDOW STEP (include/reverie_amd.h: rv_folder_*, rv_ops_fold_windows_host) that shares
no code with the library, nor with tests/fold_ref.py's sweep: plain dicts.  Between windows it holds, per domain, index -> (known,
value) for every index some op wrote (an index nobody wrote is the zero wire: known 0).  A window is stepped as the kernels step it:
every read is resolved to its last writer inside the window and before the reader, or escapes to the tables; the ops known at once
are layer 0; a known value is told to its readers layer by layer (a zero makes a Mul reader known, anything else takes one from the
reader's count of unknown in-window reads; an op with an unknown escaping read never gets there); every record is rewritten from what
is known of its reads; then the window's last writer of every index it writes sets the tables.
  fold_windows(ops, wc, cuts) -> (code, records or None, info dict, layers per window, the log [(ordinal, record tuple)])
  replay(ops, log, first, n)  -> the records [first, first + n) of the folded list, from the source's and the log
  cuttings(n, rng)            -> the cuttings the tests share"""
from __future__ import annotations

import numpy as np

OK, WIRE_OOB, BAD_OP, ARG = 0, 3, 5, 9
M64 = (1 << 64) - 1
INPUT, RANDOM, ADD, ADDC, SUB, SUBC, MUL, MULC, ASSERT, CONST = range(10)
TWO, ONE = (ADD, SUB, MUL), (ADDC, SUBC, MULC, ASSERT)
COUNTS = ("gf2_mul_to_const", "z64_mul_to_const", "gf2_mul_to_linear", "z64_mul_to_linear", "b2a_to_const", "gf2_other_rewritten",
          "z64_other_rewritten", "asserts_known_zero", "asserts_known_nonzero")


def _reads(rec):
    """-> (domain of the reads, their indices)"""
    dom, opc, _, _, a, b, _ = rec
    if dom == 2:
        return 0, [a + k for k in range(64)]
    if dom > 1:
        return 0, []
    return dom, [a, b] if opc in TWO else [a] if opc in ONE else []


def _defines(rec):
    """-> the domain of the value the record defines, or None"""
    dom, opc = rec[0], rec[1]
    if dom == 2:
        return 1
    return dom if dom <= 1 and opc != ASSERT else None


def _check(rec, n):
    dom, opc, reserved, dst, a, b, _ = rec
    if reserved:
        return BAD_OP
    if dom == 3:
        return OK
    if dom == 2:
        return WIRE_OOB if dst >= n[1] or a + 64 > n[0] else OK
    if dom > 3 or opc > CONST:
        return BAD_OP
    used = ([dst] if opc != ASSERT else []) + _reads(rec)[1]
    return WIRE_OOB if any(w >= n[dom] for w in used) else OK


def _judge(rec, kv):
    """kv: (known, value) per read -> (known, value) of the defining record"""
    dom, opc, imm = rec[0], rec[1], rec[6]
    if dom == 2:
        return (True, sum((v & 1) << k for k, (_, v) in enumerate(kv))) if all(k for k, _ in kv) else (False, 0)
    g = dom == 0
    c = imm & 1 if g else imm
    if opc == CONST:
        return True, c
    if opc in (INPUT, RANDOM):
        return False, 0
    if opc == MULC and c == 0:
        return True, 0
    if opc == MUL and any(k and v == 0 for k, v in kv):
        return True, 0
    if not all(k for k, _ in kv):
        return False, 0
    x = kv[0][1]
    y = kv[1][1] if len(kv) > 1 else c
    if opc in (ADD, ADDC):
        v = x ^ y if g else x + y
    elif opc in (SUB, SUBC):
        v = x ^ y if g else x - y
    else:
        v = x & y if g else x * y
    return True, v & M64


def _rewrite(rec, known, value, kv):
    """-> (the record afterwards, the count it adds to or None)"""
    dom, opc, _, dst, a, b, _ = rec
    d = _defines(rec)
    t = "gf2" if dom == 0 else "z64"
    if dom <= 1 and opc == ASSERT:
        return rec, (None if not kv[0][0] else "asserts_known_zero" if kv[0][1] == 0 else "asserts_known_nonzero")
    if d is None or (dom <= 1 and opc == CONST):
        return rec, None
    if known:
        count = "b2a_to_const" if dom == 2 else t + "_mul_to_const" if opc == MUL else t + "_other_rewritten"
        return (d, CONST, 0, dst, 0, 0, value), count
    if dom == 2 or opc not in TWO:
        return rec, None
    (ka, va), (kb, vb) = kv
    if ka == kb:
        return rec, None
    if opc == MUL:
        return (dom, MULC, 0, dst, b if ka else a, 0, va if ka else vb), t + "_mul_to_linear"
    if opc == ADD:
        return (dom, ADDC, 0, dst, b if ka else a, 0, va if ka else vb), t + "_other_rewritten"
    if kb:
        return (dom, SUBC, 0, dst, a, 0, vb), t + "_other_rewritten"
    if dom == 0:
        return (dom, ADDC, 0, dst, b, 0, va), t + "_other_rewritten"
    return rec, None  # Z64 c - x


def _window(recs, tables, info, first, log):
    """one window's step -> (the records afterwards, its layers)"""
    n = len(recs)
    last = [{}, {}]
    prods = []  # per op: per read, the in-window producer or None
    for i, rec in enumerate(recs):
        rd, ws = _reads(rec)
        prods.append([last[rd].get(w) for w in ws])
        d = _defines(rec)
        if d is not None:
            last[d][rec[3]] = i

    def escaped(rec, k):
        rd, ws = _reads(rec)
        return tables[rd].get(ws[k], (True, 0))

    known, value = [False] * n, [0] * n

    def read_state(i):
        return [escaped(recs[i], k) if p is None else (known[p], value[p] if known[p] else 0) for k, p in enumerate(prods[i])]

    readers = {}
    frontier = []
    for i, rec in enumerate(recs):
        if _defines(rec) is None:
            continue
        for p in prods[i]:
            if p is not None:
                readers.setdefault(p, []).append(i)
        # at once: from the escaping reads alone
        k, v = _judge(rec, [escaped(rec, j) if p is None else (False, 0) for j, p in enumerate(prods[i])])
        if k:
            known[i], value[i] = True, v
            frontier.append(i)
    layers = 0
    while frontier:
        layers += 1
        found = {}
        for p in frontier:
            for r in readers.get(p, ()):
                if not known[r] and r not in found:
                    k, v = _judge(recs[r], read_state(r))
                    if k:
                        found[r] = v
        for r, v in found.items():
            known[r], value[r] = True, v
        frontier = sorted(found)
    out = []
    for i, rec in enumerate(recs):
        now, count = _rewrite(rec, known[i], value[i], read_state(i))
        if count:
            info[count] += 1
        if now[:2] != rec[:2]:
            log.append((first + i, now))
        out.append(now)
    info["n_known"] += sum(known)
    for d in (0, 1):
        for w, i in last[d].items():
            tables[d][w] = (known[i], value[i] if known[i] else 0)
    return out, layers


def fold_windows(ops, wc, cuts):
    info = {k: 0 for k in ("n_ops", "n_rewritten", "n_known") + COUNTS}
    info["n_ops"] = len(ops)
    n = {0: int(wc[1]), 1: int(wc[0])}
    tables = [{}, {}]
    recs = [tuple(r) for r in ops.tolist()]
    out, layers, log = [], [], []
    bounds = [0] + [int(c) for c in cuts] + [len(recs)]
    if any(a > b for a, b in zip(bounds, bounds[1:])):
        return ARG, None, info, [], []
    for lo, hi in zip(bounds, bounds[1:]):
        for rec in recs[lo:hi]:
            if rec[0] == 3 and rec[2] == 0:
                n = {0: max(n[0], rec[5]), 1: max(n[1], rec[4])}
            rc = _check(rec, n)
            if rc:
                return rc, None, info, layers, log
        now, lay = _window(recs[lo:hi], tables, info, lo, log)
        out += now
        layers.append(lay)
    info["n_rewritten"] = sum(info[k] for k in COUNTS[:7])
    res = ops.copy()
    for j, rec in enumerate(out):
        if rec != recs[j]:
            res[j] = rec
    return OK, res, info, layers, log


def replay(ops, log, first, n):
    out = ops[first:first + n].copy()
    for ordinal, rec in log:
        if first <= ordinal < first + n:
            out[ordinal - first] = rec
    return out


def cuttings(n, rng, every_single=64):
    """-> [(name, cuts)]: no cut; a cut at every position (every feed 1 op); every single cut position for lists of at most
    `every_single` ops; empty windows at both ends and doubled cuts; five random cuttings"""
    out = [("whole", [])]
    if n:
        out.append(("one_op_feeds", list(range(1, n))))
    if n <= every_single:
        out += [(f"cut_{k}", [k]) for k in range(n + 1)]
    mid = sorted({n // 3, n // 2})
    out.append(("empty_ends_doubled", [0, 0] + [c for m in mid for c in (m, m)] + [n, n]))
    for k in range(5):
        count = int(rng.integers(1, 9))
        out.append((f"random_{k}", sorted(int(x) for x in rng.integers(0, n + 1, count))))
    return out
