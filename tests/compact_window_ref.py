"""Wire compaction in windows (csrc/compact_win.hip) as plain Python: the state the compactor carries from feed to feed.

A scan pass leaves one mark byte per op; a rewrite pass reads the marks and needs no look ahead.  Carried by the scan, per domain and
old wire index: the op that defined the value now on the index and that value's last reader so far (ordinal, operand slot).  Carried
by the rewrite pass: old index -> new slot of its current value, the FIFO of free slots, the fresh counter.  Within a feed the ops are
stepped in order here (the kernels do a feed in parallel; what crosses a cut is the same).  Test infrastructure: compared with
tests/compact_ref.py, and the reference for the kernels' carried state."""
from __future__ import annotations

from collections import deque

import numpy as np

from compact_ref import E_BAD_OP, E_WIRE_OOB, SHAPE
from reverie_amd.ops import DOM_B2A, DOM_GF2, DOM_SIZEHINT, DOM_Z64, OP_DTYPE

E_ARG = 1
G, Z = 0, 1
REL_A, REL_B, DEAD, TAKES, DOM_Z = 1, 2, 4, 8, 16  # the mark byte


class WindowCompactor:
    def __init__(self, wire_counts):
        self.decl = [int(wire_counts[1]), int(wire_counts[0])]  # [G, Z]
        self.n = list(self.decl)  # counts in force
        self.marks = bytearray()
        self.pins = None  # set of pinned GF(2) indices (second scan)
        self.b2a_starts = []
        self.values = [0, 0]
        self.scans = 0
        self.total = None
        self.state = "scan"
        self._scan_reset()

    def _scan_reset(self):
        self.defn = [{}, {}]  # index -> ordinal of the op that defined its value
        self.rd = [{}, {}]  # index -> (ordinal, slot) of that value's last reader so far
        self.zero = [0, 0]
        self.pos = 0

    # ---- scan pass ----
    def _check(self, op):
        dom, opc, dst, a, b = int(op["domain"]), int(op["opcode"]), int(op["dst"]), int(op["a"]), int(op["b"])
        if int(op["reserved"]) != 0:
            return E_BAD_OP
        if dom == DOM_SIZEHINT:
            self.n[G], self.n[Z] = max(self.n[G], b), max(self.n[Z], a)
        elif dom in (DOM_GF2, DOM_Z64):
            if opc not in SHAPE:
                return E_BAD_OP
            has_dst, reads = SHAPE[opc]
            nw = self.n[G if dom == DOM_GF2 else Z]
            if (has_dst and dst >= nw) or (reads >= 1 and a >= nw) or (reads >= 2 and b >= nw):
                return E_WIRE_OOB
        elif dom == DOM_B2A:
            if dst >= self.n[Z] or a + 64 > self.n[G]:
                return E_WIRE_OOB
        else:
            return E_BAD_OP
        return 0

    def _final(self, d, w):
        """the value on index w of domain d has had its last reader"""
        if w not in self.defn[d]:
            return
        r = self.rd[d].pop(w, None)
        if r is None:
            self.marks[self.defn[d][w]] |= DEAD
        else:
            self.marks[r[0]] |= REL_B if r[1] else REL_A
        del self.defn[d][w]

    def scan(self, ops):
        if self.state != "scan":
            return E_ARG
        ops = np.asarray(ops, OP_DTYPE)
        first = self.scans == 0
        if not first and self.pos + len(ops) > self.total:
            return E_ARG
        if first:
            self.marks.extend(bytes(len(ops)))
        for op in ops:
            o = self.pos
            if first:
                rc = self._check(op)
                if rc:
                    self.state = "failed"
                    return rc
            dom, opc, dst = int(op["domain"]), int(op["opcode"]), int(op["dst"])
            if dom in (DOM_GF2, DOM_Z64):
                d = G if dom == DOM_GF2 else Z
                has_dst, nr = SHAPE[opc]
                if d == Z:
                    self.marks[o] |= DOM_Z
                for k, w in enumerate((int(op["a"]), int(op["b"]))[:nr]):
                    if d == G and self.pins is not None and w in self.pins:
                        continue
                    if w not in self.defn[d]:
                        self.zero[d] = 1
                    elif self.rd[d].get(w, (None,))[0] != o:  # (a and b of one op on one value: the slot is a)
                        self.rd[d][w] = (o, k)
                if has_dst:
                    if first:
                        self.values[d] += 1
                    if not (d == G and self.pins is not None and dst in self.pins):
                        self._final(d, dst)
                        self.defn[d][dst] = o
                        self.marks[o] |= TAKES
            elif dom == DOM_B2A:
                if first:
                    self.values[Z] += 1
                    self.b2a_starts.append(int(op["a"]))
                self._final(Z, dst)
                self.defn[Z][dst] = o
                self.marks[o] |= TAKES | DOM_Z
            self.pos += 1
        return 0

    def scan_end(self):
        """-> (rc, again)"""
        if self.state != "scan" or (self.scans and self.pos != self.total):
            return E_ARG, 0
        self.total = self.pos
        self.scans += 1
        if self.scans == 1 and self.b2a_starts:  # the pins are known now: the marks come from a second scan
            self.pins = set()
            for a in self.b2a_starts:
                self.pins.update(range(a, a + 64))
            self.rank = {w: r for r, w in enumerate(sorted(self.pins))}
            self.marks = bytearray(self.total)
            self._scan_reset()
            return 0, 1
        for d in (G, Z):
            for w in list(self.defn[d]):
                self._final(d, w)
        # the fresh slots, from the marks alone: N = max over ops of (slots taken through the op - slots released before it)
        fresh = [0, 0]
        A, F = [0, 0], [0, 0]
        for m in self.marks:
            d = Z if m & DOM_Z else G
            if m & TAKES:
                A[d] += 1
                fresh[d] = max(fresh[d], A[d] - F[d])
            F[d] += bin(m & 7).count("1")
        self.P = len(self.pins) if self.pins else 0
        self.base = [self.P + self.zero[G], self.zero[Z]]
        self.counts = (self.zero[Z] + fresh[Z], self.P + self.zero[G] + fresh[G])
        self.info = dict(z64_wires=self.counts[0], gf2_wires=self.counts[1], gf2_pinned=self.P, gf2_zero_wire=self.zero[G],
                         z64_zero_wire=self.zero[Z], gf2_values=self.values[G], z64_values=self.values[Z])
        self.state = "feed"
        self._feed_reset()
        return 0, 0

    # ---- rewrite pass ----
    def _feed_reset(self):
        self.slotof = [{}, {}]
        self.fifo = [deque(), deque()]
        self.fresh = [0, 0]
        self.pos = 0

    def rewind(self):
        if self.state != "feed" or self.pos != self.total:
            return E_ARG
        self._feed_reset()
        return 0

    def feed(self, ops):
        """-> (rc, records)"""
        ops = np.asarray(ops, OP_DTYPE)
        if self.state != "feed" or self.pos + len(ops) > self.total:
            return E_ARG, None
        out = ops.copy()
        pinned = self.pins or ()
        for i, op in enumerate(ops):
            m = self.marks[self.pos]
            self.pos += 1
            dom, opc, dst = int(op["domain"]), int(op["opcode"]), int(op["dst"])
            if dom == DOM_SIZEHINT:
                out["a"][i], out["b"][i] = self.counts
                continue
            d = Z if m & DOM_Z else G
            slot = None
            if m & TAKES:
                if self.fifo[d]:
                    slot = self.fifo[d].popleft()
                else:
                    slot = self.base[d] + self.fresh[d]
                    self.fresh[d] += 1
            if dom == DOM_B2A:
                out["a"][i] = self.rank[int(op["a"])]
            else:
                for k in range(SHAPE[opc][1]):
                    w = int(op["ab"[k]])
                    if d == G and w in pinned:
                        new = self.rank[w]
                    elif w not in self.slotof[d]:
                        new = self.P if d == G else 0
                    else:
                        new = self.slotof[d][w]
                        if m & (REL_B if k else REL_A):
                            self.fifo[d].append(new)
                    out["ab"[k]][i] = new
            if slot is not None:
                if m & DEAD:
                    self.fifo[d].append(slot)
                self.slotof[d][dst] = slot
                out["dst"][i] = slot
            elif dom == DOM_GF2 and SHAPE[opc][0]:
                out["dst"][i] = self.rank[dst]
        return 0, out


def cut(ops, cuts):
    """the pieces of ops at the given offsets (empty ones where offsets repeat)"""
    edges = [0] + sorted(int(c) for c in cuts) + [len(ops)]
    return [ops[a:b] for a, b in zip(edges[:-1], edges[1:])]


def compact_windowed(ops, wire_counts, scan_cuts=(), feed_cuts=(), passes=1):
    """-> (rc, new_ops per rewrite pass, counts, info, scans)"""
    ops = np.asarray(ops, OP_DTYPE)
    c = WindowCompactor(wire_counts)
    while True:
        for part in cut(ops, scan_cuts):
            rc = c.scan(part)
            if rc:
                return rc, None, None, None, c.scans
        rc, again = c.scan_end()
        assert rc == 0
        if not again:
            break
    outs = []
    for p in range(passes):
        if p:
            assert c.rewind() == 0
        parts = []
        for part in cut(ops, feed_cuts):
            rc, o = c.feed(part)
            assert rc == 0
            parts.append(o)
        outs.append(np.concatenate(parts) if parts else np.zeros(0, OP_DTYPE))
    return 0, outs, c.counts, c.info, c.scans
