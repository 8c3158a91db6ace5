"""Record lists for the fused Z64 level kernel's launch-level tests (tests/test_z64f_ref_host.py, tests/test_gpu_z64_fused_level.py;
reference tests/z64f_ref.py) -- TEST INFRASTRUCTURE.

Two sources: production's own records of a program (fused_gates: rv_hook_z64_fused_gates, host only) and records assembled by hand
(Builder), which reach what one compiler run never yields: any first_block, any transcript offset, a preprocessing stream with gaps,
an Input row that shares its cipher block with a Mul.  Every Case passes check_independent: within one level no record reads a row, a
clear value or a correction that another record of that level writes, no two write the same one, no two share a transcript word, and no
Mul reads the row it writes -- the kernel relies on its callers for that, and rv_hook_z64_fused_run cannot check it."""
import ctypes as C
import functools

import numpy as np

import z64f_ref as zr
from z64f_ref import ADD, ADDC, ASSERT, CONST, GATE, INPUT, MASK_ROW, MUL, MULC, SUB, SUBC

M64 = (1 << 64) - 1
EDGE_VALUES = (0, 1, 1 << 63, M64)
MAX_CTR = 1 << 24
CLASS = {MUL: 0, ADD: 1, SUB: 1, ADDC: 1, SUBC: 1, MULC: 1, INPUT: 2, ASSERT: 2, CONST: 2}


class Case:
    def __init__(self, name, gates, levels, runs, n_ssa, n_rows, on_words, pre_words, wit, n_in, n_corr, n_rec):
        self.name, self.gates = name, np.ascontiguousarray(gates, GATE)
        self.levels = np.ascontiguousarray(levels, np.uint32).reshape(-1, 4)
        self.runs = np.ascontiguousarray(runs, np.uint64).reshape(-1, 2)
        self.n_ssa, self.n_rows, self.on_words, self.pre_words = int(n_ssa), int(n_rows), int(on_words), int(pre_words)
        self.wit = np.ascontiguousarray(wit, np.uint64)
        self.n_in, self.n_corr, self.n_rec = int(n_in), int(n_corr), int(n_rec)
        check_independent(self)

    def counts(self):
        return [(int(l[1] - l[0]), int(l[2] - l[1]), int(l[3] - l[2])) for l in self.levels]

    def last_block(self):
        """the highest cipher block index (relative to first_block) a record or a run reaches"""
        mul = [int(g["m"]) // 2 for g in self.gates if g["op"] == MUL]
        return max(mul + [int(f + n - 1) for f, n in self.runs])


def _touches(g):
    """(rows read, rows written, values read, values written, on words, pre words) of one record"""
    op, dst, a, b, m = (int(g[k]) for k in ("op", "dst", "a", "b", "m"))
    am, bm, eo, ep = int(g["am"]), int(g["bm"]), int(g["eo"]), int(g["ep"])
    if op == MUL:
        return {am, bm}, {MASK_ROW | (m + 1)}, {a, b}, {dst}, set(range(eo, eo + 8)), {ep}
    if op in (ADD, SUB):
        return {am, bm}, {dst}, {a, b}, {dst}, set(), set()
    if op in (ADDC, SUBC, MULC):
        return {am}, {dst}, {a}, {dst}, set(), set()
    if op == INPUT:
        return {("gen", m)}, {MASK_ROW | m}, set(), {dst}, {eo}, set()
    if op == ASSERT:
        return {am}, set(), {a}, set(), set(range(eo, eo + 8)), set()
    assert op == CONST, op
    return set(), {dst}, set(), {dst}, set(), set()


def check_independent(case):
    on_all, pre_all = set(), set()
    for lv in case.levels:
        t = [_touches(g) for g in case.gates[int(lv[0]):int(lv[3])]]
        for i, (rr, rw, vr, vw, on, pre) in enumerate(t):
            assert not (on & on_all) and not (pre & pre_all), (case.name, "two records share a transcript word")
            on_all |= on
            pre_all |= pre
            if case.gates[int(lv[0]) + i]["op"] == MUL:
                assert not (rr & rw), (case.name, "a Mul reads the row it writes")
            for j, (rr2, rw2, vr2, vw2, _, _) in enumerate(t):
                if i != j:
                    assert not (rw & (rr2 | rw2)) and not (vw & (vr2 | vw2)), (case.name, "records of one level depend on each other", i, j)
    assert max(on_all, default=-1) < case.on_words and max(pre_all, default=-1) < case.pre_words


# ---------------------------------------------------------------- production's records of a program
def fused_gates(prog, wc):
    """rv_hook_z64_fused_gates -> (gates, levels [n, 4], runs [n, 2], eligible, sizes = n_ssa, n_masks, on_words, pre_words, n_in,
    n_corr, n_rec); count first, then fill"""
    from reverie_amd import _lib

    lib = _lib.lib()
    ng, nl, nr, why = C.c_size_t(0), C.c_size_t(0), C.c_size_t(0), C.c_int(-1)
    sizes = np.zeros(7, np.uint64)
    head = (prog.ctypes.data_as(C.c_void_p), C.c_size_t(len(prog)), C.c_size_t(wc[0]), C.c_size_t(wc[1]), C.c_uint32(0))
    _lib.check(lib.rv_hook_z64_fused_gates(*head, None, 0, C.byref(ng), None, 0, C.byref(nl), None, 0, C.byref(nr), C.byref(why), None))
    gates = np.zeros(max(ng.value, 1), GATE)
    levels = np.zeros((max(nl.value, 1), 4), np.uint32)
    runs = np.zeros((max(nr.value, 1), 2), np.uint64)
    p = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    _lib.check(lib.rv_hook_z64_fused_gates(*head, p(gates), ng.value, C.byref(ng), p(levels), nl.value, C.byref(nl), p(runs), nr.value, C.byref(nr),
                                           C.byref(why), p(sizes)))
    return gates[:ng.value], levels[:nl.value], runs[:nr.value], why.value, tuple(int(s) for s in sizes)


def from_program(name, prog, wit64, wc):
    gates, levels, runs, why, (n_ssa, n_masks, on_words, pre_words, n_in, n_corr, n_rec) = fused_gates(prog, wc)
    assert why == 0, (name, why)
    levels = levels[levels[:, 3] > levels[:, 0]]  # (a level without Z64 gates is not launched)
    return Case(name, gates, levels, runs, n_ssa, (n_masks + 1) // 2 * 2, on_words, pre_words, wit64, n_in, n_corr, n_rec)


# ---------------------------------------------------------------- records by hand
class Wire:
    def __init__(self, ssa, ref, val):
        self.ssa, self.ref, self.val = ssa, ref, val & M64


class Builder:
    def __init__(self):
        self.recs, self.wit = [], []
        self.n_ssa = self.next_row = self.eo = self.ep = self.n_in = self.n_corr = self.n_rec = 0
        self.top_row = 0

    def _ssa(self, dst):
        if dst is not None:
            return dst
        self.n_ssa += 1
        return self.n_ssa - 1

    def _rec(self, level, **kw):
        g = np.zeros((), GATE)
        for k, v in kw.items():
            g[k] = v
        self.recs.append((level, CLASS[int(kw["op"])], len(self.recs), g))

    def _rows(self, m, n):
        if m is None:
            m = self.next_row + (self.next_row & 1 if n == 2 else 0)
            self.next_row = m + n
        self.top_row = max(self.top_row, m + n)
        return m

    def pad_on(self, n):
        self.eo += n

    def pad_pre(self, n):
        self.ep += n

    def inp(self, level, val, m=None, dst=None):
        m, dst = self._rows(m, 1), self._ssa(dst)
        self._rec(level, op=INPUT, dst=dst, m=m, eo=self.eo, x=self.n_in)
        self.wit.append(val & M64)
        self.eo += 1
        self.n_in += 1
        return Wire(dst, MASK_ROW | m, val)

    def const(self, level, imm, dst=None):
        dst = self._ssa(dst)
        self._rec(level, op=CONST, dst=dst, imm=imm & M64)
        return Wire(dst, dst, imm)

    def mul(self, level, a, b, m=None, dst=None):
        m, dst = self._rows(m, 2), self._ssa(dst)
        assert m % 2 == 0
        self._rec(level, op=MUL, dst=dst, a=a.ssa, b=b.ssa, am=a.ref, bm=b.ref, m=m, eo=self.eo, ep=self.ep, x=self.n_rec, xc=self.n_corr)
        self.eo += 8
        self.ep += 1
        self.n_rec += 1
        self.n_corr += 1
        return Wire(dst, MASK_ROW | (m + 1), a.val * b.val)

    def lin(self, level, op, a, b=None, imm=0, dst=None):
        dst = self._ssa(dst)
        two = op in (ADD, SUB)
        self._rec(level, op=op, dst=dst, a=a.ssa, am=a.ref, b=b.ssa if two else 0, bm=b.ref if two else 0, imm=imm & M64)
        val = {ADD: lambda: a.val + b.val, SUB: lambda: a.val - b.val, ADDC: lambda: a.val + imm, SUBC: lambda: a.val - imm, MULC: lambda: a.val * imm}[op]()
        return Wire(dst, dst, val)

    def az(self, level, a):
        self._rec(level, op=ASSERT, a=a.ssa, am=a.ref, eo=self.eo, x=self.n_rec)
        self.eo += 8
        self.n_rec += 1

    def finish(self, name, on_tail=0, pre_tail=0):
        recs = sorted(self.recs, key=lambda r: r[:3])
        gates = np.array([r[3] for r in recs], GATE)
        levels, at = [], 0
        for lv in sorted({r[0] for r in recs}):
            n = [sum(1 for r in recs if r[0] == lv and r[1] == k) for k in range(3)]
            levels.append((at, at + n[0], at + n[0] + n[1], at + sum(n)))
            at += sum(n)
        runs = []  # (csrc/api.hip: build_z64_fused)
        for blk in sorted({int(g["m"]) // 2 for g in gates if g["op"] == INPUT}):
            if runs and blk == runs[-1][0] + runs[-1][1]:
                runs[-1][1] += 1
            else:
                runs.append([blk, 1])
        n_rows = (self.top_row + 1) // 2 * 2 + 2  # (a pair of rows nobody touches behind the last)
        return Case(name, gates, levels, runs, self.n_ssa + 1, n_rows, self.eo + on_tail, max(self.ep + pre_tail, 1), self.wit, self.n_in, self.n_corr,
                    self.n_rec)


def _values(seed, n):
    rng = np.random.default_rng(seed)
    return [int(x) for x in rng.integers(0, 1 << 63, n, dtype=np.uint64) * 2 + rng.integers(0, 2, n, dtype=np.uint64)]


@functools.lru_cache(maxsize=None)
def counters(n_mul=9):
    """level 0: three Inputs on mask rows 1, 2, 3 (cipher blocks 0 and 1; row 1 is an ODD row whose block 0 is also the first Mul's);
    level 1: n_mul Muls on blocks 0, 2, 3, .., n_mul and two linear gates.  The caller moves the window with first_block."""
    assert 4 <= n_mul <= 12
    b = Builder()
    v = _values(1, 3)
    x, y, z = (b.inp(0, v[i], m=1 + i) for i in range(3))
    b.next_row = 4
    ws = [y, z]
    for i in range(n_mul):
        ws.append(b.mul(1, ws[i % 2], ws[(i + 1) % 2] if i % 3 else ws[i % 2], m=0 if i == 0 else None))
    b.lin(1, ADD, y, z)
    b.lin(1, SUBC, z, imm=7)
    c = b.finish(f"counters{n_mul}")
    assert c.last_block() == n_mul and c.runs.tolist() == [[0, 2]] and c.counts() == [(0, 0, 3), (n_mul, 2, 0)]
    return c


@functools.lru_cache(maxsize=None)
def shapes(jw):
    """every level shape the wavefront deal and the grid distinguish at JW = 64 / QW gates per wavefront step: an other-only level, a
    linear-only one, then Mul levels of 1, JW - 1, JW, JW + 1, 8 JW - 1, 8 JW + 1 and 100 gates (several chunks per quad group), bare,
    with linear gates, or with all three classes"""
    b = Builder()
    v = _values(2, 8)
    ins = [b.inp(0, v[i]) for i in range(8)] + [b.const(0, 5), b.const(0, M64)]
    lins = [b.lin(1, (ADD, SUB, ADDC, SUBC, MULC)[i % 5], ins[i % 10], ins[(3 * i + 1) % 10], imm=v[i % 8]) for i in range(11)]
    zero = b.lin(1, SUB, ins[0], ins[0])
    pool = ins + lins
    for k, n in enumerate((1, jw - 1, jw, jw + 1, 8 * jw - 1, 8 * jw + 1, 100)):
        lv = 2 + k
        for i in range(n):
            b.mul(lv, pool[(i + k) % len(pool)], pool[(5 * i + 2 * k + 1) % len(pool)])
        if k % 3:
            for i in range(3 * k + 1):
                b.lin(lv, (ADD, SUB, MULC)[i % 3], pool[(i + 4) % len(pool)], pool[(2 * i + 1) % len(pool)], imm=3)
        if k % 3 == 2:
            b.az(lv, zero)
            b.const(lv, 9 + k)
    c = b.finish(f"shapes{jw}")
    assert [x[0] for x in c.counts()] == [0, 0, 1, jw - 1, jw, jw + 1, 8 * jw - 1, 8 * jw + 1, 100]
    assert c.counts()[0][:2] == (0, 0) and c.counts()[1] == (0, 12, 0) and c.counts()[2] == (1, 0, 0) and all(c.counts()[4])
    return c


@functools.lru_cache(maxsize=None)
def placement(on_pad, on_tail, pre_layout):
    """transcript placement: on_pad words in front of the first record make every eo odd or even, on_tail makes on_words (the stride
    between two repetitions' streams) odd or even.  Ten Muls = two full wavefront steps of four and one with two gates missing at
    QW 16: pre_layout "run" leaves their ep consecutive, "gap" puts a hole behind the sixth Mul (inside the second step)."""
    b = Builder()
    v = _values(3, 4)
    b.pad_on(on_pad)
    ins = [b.inp(0, v[i]) for i in range(4)]
    one = b.const(0, 1)
    z = b.lin(1, SUB, ins[0], ins[0])
    for i in range(10):
        b.mul(1, ins[i % 4], ins[(i + 1) % 4] if i % 2 else one)
        if pre_layout == "gap" and i == 5:
            b.pad_pre(3)
    b.az(2, z)
    b.az(2, ins[1])  # (shares, not a check of the value: the prover's error word must show it, see the tests)
    c = b.finish(f"placement-{on_pad}-{on_tail}-{pre_layout}", on_tail=on_tail, pre_tail=1)
    assert c.counts() == [(0, 0, 5), (10, 1, 0), (0, 0, 2)]
    return c


@functools.lru_cache(maxsize=None)
def operands(bad_assert):
    """operand forms and edge values: am / bm as a wmask row and as a generator row, a == b, a dst that an earlier level read as an
    operand, values and immediates 0, 1, 2^63, 2^64 - 1, MulConst by 0, AssertZero on zero rows (and, bad_assert, on the value 1)"""
    b = Builder()
    v = list(EDGE_VALUES) + _values(4, 4)
    i = [b.inp(0, x) for x in v]
    c = [b.const(0, x) for x in EDGE_VALUES]
    lin1 = [b.lin(1, ADD, i[0], i[1]), b.lin(1, SUB, i[2], i[3]), b.lin(1, ADDC, i[4], imm=M64), b.lin(1, MULC, i[7], imm=1 << 63),
            b.lin(1, ADD, c[0], i[4]), b.lin(1, SUB, c[3], c[2]), b.lin(1, ADDC, c[1], imm=0), b.lin(1, SUBC, i[3], imm=1)]
    z = [b.lin(1, SUBC, i[5], imm=i[5].val), b.lin(1, MULC, i[6], imm=0), b.lin(1, SUB, i[1], i[1])]
    m1 = [b.mul(1, i[0], i[1]), b.mul(1, c[1], i[2]), b.mul(1, i[3], c[3]), b.mul(1, i[4], i[4]), b.mul(1, c[2], c[2]), b.mul(1, i[2], i[3]),
          b.mul(1, c[0], i[5])]
    assert all(w.val == 0 for w in z)
    # level 2: dst = the SSA id of a Const that level 1 read (its wmask row, its value and its correction are overwritten)
    r0 = b.lin(2, MULC, m1[0], imm=3, dst=c[0].ssa)
    r1 = b.mul(2, lin1[0], m1[1], dst=c[1].ssa)
    r2 = b.lin(2, ADD, lin1[3], m1[4], dst=c[2].ssa)
    for w in z:
        b.az(2, w)
    if bad_assert:
        b.az(2, i[1])
    m2 = [b.mul(2, m1[2], lin1[1]), b.mul(2, m1[3], m1[3]), b.mul(2, lin1[5], lin1[6])]
    t = [b.lin(3, SUBC, w, imm=w.val) for w in (r0, r1, r2, m2[0], m2[1], m2[2])]
    for w in t:
        b.az(4, w)
    return b.finish("operands-bad" if bad_assert else "operands")


# ---------------------------------------------------------------- the verifier's inputs
def omits(R, kind):
    """none: nobody opened.  mix: a fixed-seed mix of players and 8 in which every player occurs, with quad word 1 (repetitions 4..7)
    opened whole and both neighbours of every edge between two quad groups opened"""
    if kind == "none":
        return np.full(R, 8, np.uint8)
    assert kind == "mix"
    rng = np.random.default_rng(500 + R)
    o = np.concatenate([np.arange(9), rng.integers(0, 9, R - 9)]).astype(np.uint8)
    rng.shuffle(o)
    o[4:8] = (3, 0, 7, 5)
    per = 4 * zr.qw_of(R // 4)
    for e in range(per, R, per):
        o[e - 1], o[e] = 2, 6
    assert set(o.tolist()) == set(range(9))
    return o


def honest_sup(case, prover, omit, seed=9):
    """the values a proof would carry, from the prover reference's transcripts, by ordinal: [n][R] each; what no honest verifier reads
    (unopened repetitions) is random"""
    R = prover.R
    rng = np.random.default_rng(seed)
    sup = [rng.integers(0, 1 << 63, (max(n, 1), R), dtype=np.uint64) for n in (case.n_in, case.n_corr, case.n_rec)]
    opened = np.flatnonzero(omit < 8)
    for g in case.gates:
        op, eo = int(g["op"]), int(g["eo"])
        if op == INPUT:
            sup[0][g["x"], opened] = prover.on[opened, eo]
        if op == MUL:
            sup[1][g["xc"], opened] = prover.pre[opened, int(g["ep"])]
        if op in (MUL, ASSERT):
            sup[2][g["x"], opened] = prover.on[opened, eo + omit[opened].astype(np.int64)]
    return sup


_BLOCKS = {}  # (seeds, omit) -> {counter: rows}: the cipher blocks of one key set, shared by every reference run under it


def run_ref(case, seeds, omit, first_block, qg0=0, qgn=None, sup=None):
    kw = dict(zip(("sup_in", "sup_corr", "sup_rec"), sup)) if sup is not None else {}
    st = zr.Level(seeds=seeds, omit=omit, first_block=first_block, n_ssa=case.n_ssa, n_rows=case.n_rows, on_words=case.on_words,
                  pre_words=case.pre_words, wit=case.wit, **kw)
    if len(_BLOCKS) > 64:
        _BLOCKS.clear()
    st._ks = _BLOCKS.setdefault((st.seeds.tobytes(), None if omit is None else st.omit.tobytes()), {})
    return zr.run(case.gates, case.levels, case.runs, qg0, qgn, state=st)
