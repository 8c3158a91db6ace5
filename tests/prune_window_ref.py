"""A Python model of the window step of the windowed pruning (include/reverie_amd.h: rv_pruner_*), in the device's
order of work -- resolve, count, live-out, peel, kill, gen -- that shares no code with the library and with tests/prune_ref.py only
`shape`, the reading of one record.

  window_step(ops, N)               one window against the needed sets N = [set, set] as they stand at its end; N is changed to what it
                                    is at the window's beginning -> (keep flags, info dict of the class counts, layers peeled)
  prune_windows(ops, cuts, og, oz)  the mark pass over the windows [0, cuts[0]), [cuts[0], cuts[1]), .. from the last to the first
                                    -> (keep flags of the whole list, info dict with "device_rounds" the summed layers)
  cuttings(n, rng)                  the ways of cutting a list of n ops the tests go through"""
from __future__ import annotations

import numpy as np

from prune_ref import CLASSES, G, Z, shape


def window_step(ops, N):
    shapes = [shape(r) for r in ops.tolist()]
    n = len(shapes)
    # 1. every read to the last writer of its index inside the window and before the reader; the others escape
    cur = [{}, {}]
    reads_of = [[] for _ in range(n)]
    escapes = [[] for _ in range(n)]
    count = [0] * n
    for i, (d, dst, rd, reads, _, _) in enumerate(shapes):
        for w in reads:
            v = cur[rd].get(w)
            if v is None:
                escapes[i].append(w)
            else:
                reads_of[i].append(v)
                count[v] += 1  # 2. one per resolved read
        if d is not None:
            cur[d][dst] = i
    # 2. the live-out: the window's last writer of a needed index
    for d in (G, Z):
        for w, v in cur[d].items():
            if w in N[d]:
                count[v] += 1
    # 3. the peeling
    keep = np.ones(n, bool)
    frontier = [i for i, s in enumerate(shapes) if s[0] is not None and not s[4] and count[i] == 0]
    layers = 0
    while frontier:
        layers += 1
        nxt = []
        for i in frontier:
            keep[i] = False
            for v in reads_of[i]:
                count[v] -= 1
                if count[v] == 0 and not shapes[v][4]:
                    nxt.append(v)
        frontier = nxt
    # 4. the Inputs whose count stayed 0
    info = {k: 0 for k in CLASSES}
    for i, s in enumerate(shapes):
        if not keep[i]:
            info[s[5]] += 1
        elif s[0] is not None and s[4] and count[i] == 0:
            info["unread_gf2_inputs" if s[0] == G else "unread_z64_inputs"] += 1
    # 5. kill, then gen
    for d in (G, Z):
        N[d] -= set(cur[d])
    for i, (_, _, rd, _, _, _) in enumerate(shapes):
        if keep[i]:
            N[rd].update(escapes[i])
    return keep, info, layers


def prune_windows(ops, cuts, outs_gf2=(), outs_z64=()):
    n = len(ops)
    bounds = [0] + [int(c) for c in cuts] + [n]
    N = [set(int(w) for w in outs_gf2), set(int(w) for w in outs_z64)]
    keep = np.zeros(n, bool)
    info = {k: 0 for k in CLASSES}
    rounds = 0
    for k in range(len(bounds) - 2, -1, -1):
        lo, hi = bounds[k], bounds[k + 1]
        keep[lo:hi], part, layers = window_step(ops[lo:hi], N)
        for name in CLASSES:
            info[name] += part[name]
        rounds += layers
    info["n_kept"] = int(np.count_nonzero(keep))
    info["n_dropped"] = n - info["n_kept"]
    info["device_rounds"] = rounds
    return keep, info


def cuttings(n, rng, every_cut_below=15, n_random=2):
    """lists of cut positions for a list of n ops: no cut; at 1 and n - 1; on and one past every multiple of 256; random cuts; and on
    a small list every single cut and all cuts at once"""
    out = [[]]
    if n >= 2:
        out.append(sorted({1, n - 1}))
    m = sorted({c for k in range(256, n, 256) for c in (k, k + 1) if c < n})
    if m:
        out.append(m)
    for _ in range(n_random if n >= 3 else 0):
        out.append(sorted(rng.integers(0, n + 1, int(rng.integers(1, 6))).tolist()))
    if 1 < n < every_cut_below:
        out += [[c] for c in range(1, n)]
        out.append(list(range(1, n)))
    return out
