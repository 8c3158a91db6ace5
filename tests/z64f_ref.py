"""Plain numpy reference of ONE fused Z64 level launch (csrc/aes.hip: k_z64_fused) -- TEST INFRASTRUCTURE.

Written from the protocol, not from the kernel: Instance::step / op_mul at Z64 (interpreter/single.rs), the prover's transcript records
(transcript/prover.rs:181-232), the verifier's two transcripts (verifier/online.rs:122-183, verifier/preprocess.rs:46-79), the share
generator (generator/share.rs:54-65 through tests/maskgen_ref.py, which is tied to the oracle) and DESIGN.md.  Arithmetic is
numpy.uint64, i.e. modulo 2^64.  tests/test_z64f_ref_host.py ties this module to the oracle's commitments before any GPU result is
compared with it.

Everything here is in the NATURAL order: a row is [repetition][player], R x 8 words.  One gate, repetition r, players p = 0..7, with
l_x[p] the mask share of wire x and S(x) = sum over p of l_x[p]:

  Input d (mask row m, ordinal x)       l_d = fresh row m.  Prover: on[eo] = wit[x] - S(d).  Verifier: on[eo] = corr(d) = the supplied
                                        input sup_in[x] in an opened repetition, 0 in the others.
  Add / Sub / AddConst / SubConst /     shares player by player (a constant moves no share, MulConst scales every share); the clear
  MulConst                              value (prover) or the public correction (verifier) alike.
  Const d, c                            l_d = 0; value / correction c.
  Mul d = a * b (mask rows m, m + 1)    l_ab = fresh row m, l_d = fresh row m + 1, both the cipher block first_block + m // 2.
                                        corr(x) = value(x) - S(x) (prover) or the public correction (verifier).
                                        on[eo + p] = l_b[p] corr(a) + l_a[p] corr(b) + l_ab[p] - l_d[p]
                                        pre[ep] = S(a) S(b) - S(ab)
                                        Verifier, opened repetition hiding player o: every share of o counts as zero, pre[ep] is the
                                        supplied correction sup_corr[xc], on[eo + o] gains the supplied share sup_rec[x], and
                                        corr(d) = sum of the eight on words + pre[ep] + corr(a) corr(b); a repetition that is not
                                        opened: corr(d) = pre[ep] + corr(a) corr(b) (junk that only keeps the stream lengths).
  AssertZero a (ordinal x)              on[eo + p] = l_a[p] (verifier, opened: player o's word is sup_rec[x]).  Prover: value(a) != 0
                                        sets RV_E_WITNESS_INVALID in err.  Verifier, opened: corr(a) + the eight words != 0 sets the
                                        zero-check bit 0x100.

What a launch over quad groups [qg0, qg0 + qgn) writes -- the rest of every buffer is left alone: the repetitions of those groups
(4 QW repetitions each) in wmask / masks rows, wcorr, on and pre; v (the prover's clear values, one per SSA id) only when the range holds
quad word 0, i.e. qg0 == 0; err whenever a check fires.

THE STORED LAYOUT.  The fused path keeps its rows piece-major inside a block of QW quad words (QW = 16 when the row's NQ quad words
are a multiple of 16, else 8): piece i (slots 2 i, 2 i + 1 of a quad word's 32 slots; slot = 8 (r % 4) + player) of quad word ql of
group qg sits at u64 offset  qg * 32 QW + i * 2 QW + ql * 2.  `stored_index` states that map once; it is used only to convert buffers.
The Input rows are the exception: the stand-alone generator writes them in the natural order for EVERY quad group before the first
level, and the Input gate rewrites the groups of its launch in the stored layout.  `natural[row, group]` remembers which."""
from __future__ import annotations

import numpy as np

import maskgen_ref
import oracle_lib

INPUT, ADD, SUB, ADDC, SUBC, MULC, MUL, ASSERT, RANDOM, CONST, B2A = range(11)
MASK_ROW = 0x80000000
E_WITNESS_INVALID, DEV_ZERO_CHECK = 1, 0x100
FILL = np.uint64(0xA5A5A5A5A5A5A5A5)
# csrc/internal.h: Gate64
GATE = np.dtype([("op", "<u4"), ("dst", "<u4"), ("a", "<u4"), ("b", "<u4"), ("m", "<u4"), ("m2", "<u4"), ("eo", "<u8"), ("ep", "<u8"),
                 ("x", "<u4"), ("xc", "<u4"), ("imm", "<u8"), ("am", "<u4"), ("bm", "<u4")])
assert GATE.itemsize == 64


def qw_of(NQ):
    return 16 if NQ % 16 == 0 else 8 if NQ % 8 == 0 else 0


def stored_index(NQ):
    """P with stored_row[P[n]] = natural_row[n] for the NQ * 32 words of a row"""
    QW = qw_of(NQ)
    assert QW
    n = np.arange(NQ * 32)
    q, s = n // 32, n % 32
    qg, ql, i, j = q // QW, q % QW, s // 2, s % 2
    return qg * 32 * QW + i * 2 * QW + ql * 2 + j


class Level:
    """the buffers of a run of fused level launches, natural order; `omit` None: the prover"""

    def __init__(self, seeds, omit, first_block, n_ssa, n_rows, on_words, pre_words, wit=(), sup_in=None, sup_corr=None, sup_rec=None):
        self.seeds = np.asarray(seeds, np.uint8).reshape(-1, 16)
        self.R = R = len(self.seeds)
        self.NQ, self.QW = R // 4, qw_of(R // 4)
        assert R % 4 == 0 and self.QW
        self.omit = None if omit is None else np.asarray(omit, np.uint8)
        self.verify = omit is not None
        self.first_block = int(first_block)
        self.keys = np.stack([oracle_lib.expand_seed(s) for s in self.seeds])
        self.wmask = np.full((n_ssa, R, 8), FILL)
        self.masks = np.full((n_rows, R, 8), FILL)
        self.natural = np.zeros((n_rows, self.NQ // self.QW), bool)
        self.v = np.full(n_ssa, FILL)
        self.wcorr = np.full((n_ssa, R), FILL)
        self.on = np.full((R, on_words), FILL)
        self.pre = np.full((R, pre_words), FILL)
        self.err = 0  # (the error word starts clear: 0xA5A5A5A5 holds both bits a check can set)
        self.wit = np.asarray(wit, np.uint64)
        z = np.zeros((0, R), np.uint64)
        self.sup_in, self.sup_corr, self.sup_rec = (z if s is None else np.asarray(s, np.uint64) for s in (sup_in, sup_corr, sup_rec))
        self._ks = {}

    # ---- fresh masks
    def block(self, ctr):
        """rows 2 j, 2 j + 1 of cipher block j at counter `ctr`: [2, R, 8]"""
        if ctr not in self._ks:
            assert 0 <= ctr < (1 << 24), ctr
            ks = maskgen_ref.keystream_from_keys(self.keys, self.omit, ctr, 1)
            self._ks[ctr] = maskgen_ref.z64_rows(ks).reshape(2, self.R, 8)
        return self._ks[ctr]

    def generate(self, runs):
        """the Input rows' generator launches: every block run, every quad group, natural order"""
        for first, n in runs:
            for j in range(int(first), int(first + n)):
                self.masks[2 * j:2 * j + 2] = self.block(self.first_block + j)
                self.natural[2 * j:2 * j + 2] = True

    # ---- rows
    def _row(self, ref, groups):
        ref = int(ref)
        if ref & MASK_ROW:
            assert not self.natural[ref & ~MASK_ROW, groups].any(), "an operand row still in the generator's order (no Input gate ran on it)"
            return self.masks[ref & ~MASK_ROW]
        return self.wmask[ref]

    def level(self, gates, qg0, qgn):
        """one launch: `gates` (GATE records, any order within the level) over quad groups [qg0, qg0 + qgn)"""
        if not qgn or not len(gates):
            return
        per = 4 * self.QW
        rs = slice(qg0 * per, (qg0 + qgn) * per)
        groups = slice(qg0, qg0 + qgn)
        reps = np.arange(rs.start, rs.stop)
        writer = qg0 == 0 and not self.verify
        V = self.verify
        opened = self.omit[rs] < 8 if V else None
        hid = self.omit[rs][opened].astype(np.int64) if V else None
        orep = reps[opened] if V else None
        with np.errstate(over="ignore"):
            for g in gates:
                op, dst, a, b, m, eo, ep = (int(g[k]) for k in ("op", "dst", "a", "b", "m", "eo", "ep"))
                imm = np.uint64(g["imm"])
                if op == MUL:
                    assert m % 2 == 0
                    lab, lnew = (r[rs] for r in self.block(self.first_block + m // 2))
                    la, lb = self._row(g["am"], groups)[rs].copy(), self._row(g["bm"], groups)[rs].copy()
                    sa, sb = la.sum(1), lb.sum(1)
                    cx, cy = (self.wcorr[a, rs].copy(), self.wcorr[b, rs].copy()) if V else (self.v[a] - sa, self.v[b] - sb)
                    w = lb * cx[:, None] + la * cy[:, None] + lab - lnew
                    delta = sa * sb - lab.sum(1)
                    if V:
                        delta[opened] = self.sup_corr[g["xc"], orep]
                        w[np.flatnonzero(opened), hid] += self.sup_rec[g["x"], orep]
                        self.wcorr[dst, rs] = np.where(opened, w.sum(1), np.uint64(0)) + delta + cx * cy
                    self.on[rs, eo:eo + 8] = w
                    self.pre[rs, ep] = delta
                    self.masks[m + 1, rs] = lnew
                    self.natural[m + 1, groups] = False
                    if writer:
                        self.v[dst] = self.v[a] * self.v[b]
                elif op in (ADD, SUB, ADDC, SUBC, MULC):
                    la = self._row(g["am"], groups)[rs]
                    f = {ADD: lambda x, y: x + y, SUB: lambda x, y: x - y, ADDC: lambda x, y: x + imm, SUBC: lambda x, y: x - imm,
                         MULC: lambda x, y: x * imm}[op]
                    two = op in (ADD, SUB)
                    lb = self._row(g["bm"], groups)[rs] if two else None
                    self.wmask[dst, rs] = la + lb if op == ADD else la - lb if op == SUB else la * imm if op == MULC else la
                    if V:
                        self.wcorr[dst, rs] = f(self.wcorr[a, rs], self.wcorr[b, rs] if two else None)
                    elif writer:
                        self.v[dst] = f(self.v[a], self.v[b] if two else None)
                elif op == INPUT:
                    assert self.natural[m, groups].all(), "an Input gate on a row the generator did not just write"
                    l = self.masks[m, rs]
                    if V:
                        corr = np.where(opened, self.sup_in[g["x"], reps] if len(self.sup_in) else np.uint64(0), np.uint64(0))
                        self.wcorr[dst, rs] = corr
                        self.on[rs, eo] = corr
                    else:
                        self.on[rs, eo] = self.wit[g["x"]] - l.sum(1)
                        if writer:
                            self.v[dst] = self.wit[g["x"]]
                    self.natural[m, groups] = False
                elif op == ASSERT:
                    l = self._row(g["am"], groups)[rs].copy()
                    if V:
                        l[np.flatnonzero(opened), hid] += self.sup_rec[g["x"], orep]
                        if ((self.wcorr[a, rs] + l.sum(1))[opened] != 0).any():
                            self.err |= DEV_ZERO_CHECK
                    elif writer and self.v[a] != 0:
                        self.err |= E_WITNESS_INVALID
                    self.on[rs, eo:eo + 8] = l
                elif op == CONST:
                    self.wmask[dst, rs] = 0
                    if V:
                        self.wcorr[dst, rs] = imm
                    elif writer:
                        self.v[dst] = imm
                else:
                    raise ValueError(f"the fused path takes no gate of op {op}")

    # ---- the device's view
    def stored(self):
        """every buffer as the device holds it: {name: array}"""
        P = stored_index(self.NQ)
        S = self.R * 8
        wmask = np.empty((len(self.wmask), S), np.uint64)
        wmask[:, P] = self.wmask.reshape(-1, S)
        nat = self.masks.reshape(-1, S)
        masks = np.empty_like(nat)
        masks[:, P] = nat
        per = 32 * self.QW
        for row, grp in np.argwhere(self.natural):
            masks[row, grp * per:(grp + 1) * per] = nat[row, grp * per:(grp + 1) * per]
        out = {"wmask": wmask, "masks": masks, "on": self.on.copy(), "pre": self.pre.copy(), "err": np.array([self.err], np.int32)}
        out["wcorr" if self.verify else "v"] = self.wcorr.copy() if self.verify else self.v.copy()
        return out

    def load_stored(self, wmask=None, masks=None):
        """initial images given in the stored layout (rows an earlier run left behind)"""
        P = stored_index(self.NQ)
        if wmask is not None:
            self.wmask[:] = np.asarray(wmask, np.uint64).reshape(len(self.wmask), -1)[:, P].reshape(self.wmask.shape)
        if masks is not None:
            self.masks[:] = np.asarray(masks, np.uint64).reshape(len(self.masks), -1)[:, P].reshape(self.masks.shape)


def run(gates, levels, runs, qg0=0, qgn=None, **kw):
    """a whole hook call: the generator launches, then every level of the table in order -> the Level"""
    st = kw.pop("state", None) or Level(**kw)
    st.generate(runs)
    n_qg = st.NQ // st.QW
    for lv in np.asarray(levels).reshape(-1, 4):
        st.level(gates[int(lv[0]):int(lv[3])], qg0, n_qg - qg0 if qgn is None else qgn)
    return st


def first_diff(name, got, want):
    idx = np.argwhere(got != want)
    if not len(idx):
        return f"{name}: equal"
    at = tuple(int(x) for x in idx[0])
    return f"{name}{list(at)}: got 0x{int(got[at]):x}, want 0x{int(want[at]):x}; {len(idx)} of {got.size} words differ"
