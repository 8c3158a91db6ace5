"""Z64 programs whose compiled levels hold a chosen number of gates of every kind, for the tests that aim at one Z64 level executor
at a time (csrc/aes.hip: k_z64_fused, csrc/z64.hip: k_interp64 / k_interp64_b): test_class_mix64_host.py proves on the host compiler
alone that every spec compiles to exactly its counts and hits the split it is named for, test_gpu_level_classes64.py runs the same
specs against the oracle.

class_mix64(levels, seed, values, order, inputs) -> (prog, witness, wire_counts).  levels[l] = L(mul=, add=, sub=, addc=, subc=, mulc=,
az=, inp=, const=): the gates of dependency level l -- Mul; the five linear ops; AssertZero; and on level 0 alone Input and Const.

Why a spec compiles to its counts: the Z64 compiler levels plainly (csrc/compile.cpp) -- a gate sits one level behind its latest
operand, nothing is folded or dropped, Input and Const sit on level 0 -- so every gate of level l takes one operand written by level
l - 1 (its "fresh" operand) and the other from any earlier level.

Every row a gate writes is read again by a live gate of a later level, rows nobody has read yet first; a gate whose result nothing reads
could compute anything.  What is still unread behind the last level goes to the sink the generator appends: SubConst(row, its clear
value) one level behind the last and AssertZero behind that (an unread row of an older level first passes through a Sub with a row
of the last level, so that the sink stands behind the last level and changes no level of the spec: three sink levels then).
class_table() reports the levels with the sink.  An AssertZero of level l reads a zero-valued row of level l - 1: the generator makes
the first SubConst gates (else Sub, MulConst, AddConst; on level 0 the first Const, else Input) of that level produce them, one per
AssertZero while there are such gates, and refuses a spec without any.

Operand forms rotate with the gate's index in its kind: the fresh operand as a or as b, a == b (Mul, Add, Sub), the destination wire
index equal to a's or to b's (the old row is then gone: nothing reads it afterwards), and for either operand a fresh mask row (the
result of an Input or a Mul, read directly) or a wmask row (the result of a linear gate or a Const) -- `coverage()` reports which
(op, kind of a, kind of b, form) occurred.

values="edges": witnesses, Const values and immediates from {0, 1, 2^32 - 1, 2^32, 2^63, 2^64 - 1} and their negations, the first
MulConst of a level by 0 and the second by 2^64 - 1; clear values are Python integers mod 2^64 in either mode ("random": 64 random bits
for every witness, constant and immediate).
order="interleaved": the gates of levels 1 and 2, 3 and 4, ... alternate in program order (each gate of the later level as soon as
its operands are there), so consecutive Mul gates of a level are not consecutive in the preprocessing transcript (no destination
wire is reused in this order).
inputs="pairs": level 0's Inputs in front of everything, an even number; "odd": an odd number (the first Mul's mask pair then
straddles two cipher blocks); ("runs", k): 2 k Inputs in k pairs with one Mul of level 1 between two pairs, k separate cipher block
runs of Input masks with block-aligned Muls."""
import collections
import functools
import itertools
import random

from reverie_amd.ops import OP_MUL, Z64, program

M64 = (1 << 64) - 1
KINDS = ("mul", "add", "sub", "addc", "subc", "mulc", "az", "inp", "const")
_E = (0, 1, (1 << 32) - 1, 1 << 32, 1 << 63, M64)
EDGES = tuple(sorted(set(_E) | {(-e) & M64 for e in _E}))
LIN_BIAS = 3  # (csrc/aes.hip: z64_fused_grid)


def L(**kw):
    """a level spec: the count of every kind of gate, in the order of KINDS"""
    assert set(kw) <= set(KINDS), kw
    return tuple(int(kw.get(k, 0)) for k in KINDS)


def bounds(lv):
    """(Mul, linear, other) of a level spec: the classes of Z64FLevel"""
    return lv[0], sum(lv[1:6]), sum(lv[6:9])


class _Row:
    __slots__ = ("wire", "val", "kind", "level", "gid", "alive", "unread")

    def __init__(self, wire, val, kind, level, gid):
        self.wire, self.val, self.kind, self.level, self.gid = wire, val, kind, level, gid
        self.alive = self.unread = True


class _Gen:
    def __init__(self, seed, values, inplace_ok):
        self.rng = random.Random(seed)
        self.values, self.inplace_ok = values, inplace_ok
        self.gates = []    # (level, op tuple, gate ids it depends on, witness or None)
        self.n_wires = 0
        self.rows = []     # every row of the finished levels
        self.unread = collections.deque()
        self.level_rows = []
        self.n_alive = 0
        self.table = []
        self.cov = set()
        self.flags = set()

    # ---- values
    def value(self):
        return self.rng.choice(EDGES) if self.values == "edges" else self.rng.getrandbits(64)

    # ---- rows
    def gate(self, l, op, deps, wit=None):
        self.gates.append((l, op, frozenset(deps), wit))
        return len(self.gates) - 1

    def new_row(self, l, wire, val, kind, gid):
        r = _Row(wire, val & M64, kind, l, gid)
        self.level_rows[l].append(r)
        return r

    def wire(self):
        self.n_wires += 1
        return self.n_wires - 1

    def begin_level(self, l):
        self.level_rows.append([])
        if l == 0:
            return
        prev = self.level_rows[l - 1]
        self.pu = {k: collections.deque(r for r in prev if r.kind == k) for k in "mw"}
        self.pa = {k: [r for r in prev if r.kind == k] for k in "mw"}
        self.rr = {"m": 0, "w": 0}
        self.alive_prev = len(prev)
        # (interleaved: a gate of the later level of a pair waits for no gate of the earlier one but its fresh operand's, see emit)
        self.older_max = l - 1 if self.inplace_ok or l < 2 else l - 2
        if not prev:
            raise ValueError(f"level {l}: level {l - 1} writes no row for its gates to stand behind")

    def end_level(self, l):
        for r in self.level_rows[l]:
            self.rows.append(r)
            self.unread.append(r)
        self.n_alive += len(self.level_rows[l])

    def fresh(self, kind):
        """a row of the previous level: one nobody has read first, of the asked kind if there is one"""
        for k in (kind, "w" if kind == "m" else "m"):
            dq = self.pu[k]
            while dq:
                r = dq.popleft()
                if r.alive and r.unread:
                    return r
            lst = self.pa[k]
            for _ in range(len(lst)):
                r = lst[self.rr[k] % len(lst)]
                self.rr[k] += 1
                if r.alive:
                    return r
        raise ValueError("no row of the previous level is left")

    def older(self, taken, kind=None):
        """a row of any finished level other than `taken`: one nobody has read first, of the asked kind if one is near"""
        while self.unread and not (self.unread[0].alive and self.unread[0].unread):
            self.unread.popleft()
        ok = lambda r: r.alive and r is not taken and r.level <= self.older_max  # noqa: E731
        near = [r for r in itertools.islice(self.unread, 0, 8) if r.unread and ok(r)]
        for r in near:
            if kind in (None, r.kind):
                return r
        if near and not any(r.kind == kind for r in self.rows[-64:]):
            return near[0]
        for n in range(64):
            r = self.rows[self.rng.randrange(len(self.rows))]
            if ok(r) and (n >= 32 or kind in (None, r.kind)):
                return r
        for r in self.rows:
            if ok(r):
                return r
        raise ValueError("too few rows for two distinct operands")

    def kill_ok(self, r, l, az_here):
        if not self.inplace_ok or (az_here and r.val == 0):
            return False
        if r.level == l - 1 and self.alive_prev <= 4:
            return False
        return self.n_alive > 12  # (rows enough for the gates behind)

    def kill(self, r, l):
        r.alive = False
        self.n_alive -= 1
        if r.level == l - 1:
            self.alive_prev -= 1

    # ---- gates
    def binary(self, l, op, i, az_here, zero=False):
        form = ("ab", "ba", "same", "dst_a", "dst_b")[(i + l) % 5]
        ka = "m" if op == "mul" and not self.inplace_ok else "mw"[i & 1]  # (interleaved: a Mul stands behind a Mul, see emit)
        p = self.fresh(ka)
        if zero:
            form = "same"  # Sub(x, x): the zero row an AssertZero of the next level reads
        if form == "same":
            a = b = p
        else:
            o = self.older(p, "mw"[(i >> 1) & 1])
            a, b = (o, p) if form == "ba" else (p, o)
        a.unread = b.unread = False
        va, vb = a.val, b.val
        val = va * vb if op == "mul" else va + vb if op == "add" else va - vb
        if op == "sub" and va < vb:
            self.flags.add("sub_wraps")
        dst = None
        if form in ("dst_a", "dst_b"):
            t = a if form == "dst_a" else b
            if self.kill_ok(t, l, az_here):
                dst = t.wire
                self.kill(t, l)
            else:
                form = "ab"
        if dst is None:
            dst = self.wire()
        self.cov.add((op, a.kind, b.kind, form))
        mk = {"mul": Z64.Mul, "add": Z64.Add, "sub": Z64.Sub}[op]
        gid = self.gate(l, mk(dst, a.wire, b.wire), {a.gid, b.gid})
        return self.new_row(l, dst, val, "m" if op == "mul" else "w", gid)

    def unary(self, l, op, i, az_here, zero=False):
        a = self.fresh("mw"[i & 1])
        a.unread = False
        imm = self.value()
        if op == "mulc" and self.values == "edges" and i < 2:
            imm = (0, M64)[i]
        if zero:
            imm = {"subc": a.val, "addc": (-a.val) & M64, "mulc": 0}[op]
        if op == "mulc":
            self.flags.add("mulc_0" if imm == 0 else "mulc_max" if imm == M64 else "mulc")
        val = a.val + imm if op == "addc" else a.val - imm if op == "subc" else a.val * imm
        form = "dst_a" if (i + l) % 3 == 2 and self.kill_ok(a, l, az_here) else "a"
        if form == "dst_a":
            dst = a.wire
            self.kill(a, l)
        else:
            dst = self.wire()
        self.cov.add((op, a.kind, "-", form))
        mk = {"addc": Z64.AddConst, "subc": Z64.SubConst, "mulc": Z64.MulConst}[op]
        gid = self.gate(l, mk(dst, a.wire, imm), {a.gid})
        return self.new_row(l, dst, val, "w", gid)

    def level0(self, lv, need_zero, odd_ok):
        c = dict(zip(KINDS, lv))
        if any(c[k] for k in KINDS[:7]):
            raise ValueError("level 0 holds Input and Const gates only")
        if c["inp"] % 2 and not odd_ok:
            raise ValueError("Inputs come in pairs (inputs='odd' takes an odd number)")
        self.begin_level(0)
        for i in range(c["const"]):
            v = 0 if need_zero and i == 0 else self.value()
            w = self.wire()
            self.new_row(0, w, v, "w", self.gate(0, Z64.Const(w, v), ()))
        for i in range(c["inp"]):
            v = 0 if need_zero and not c["const"] and i == 0 else self.value()
            w = self.wire()
            self.new_row(0, w, v, "m", self.gate(0, Z64.Input(w), (), wit=v))
        if need_zero and not (c["const"] or c["inp"]):
            raise ValueError("level 0 is empty")
        self.end_level(0)
        self.table.append(tuple(lv))

    def level(self, l, lv, need_zero):
        c = dict(zip(KINDS, lv))
        if c["inp"] or c["const"]:
            raise ValueError("Input and Const gates belong to level 0")
        self.begin_level(l)
        az_here = c["az"] > 0
        zero_op = next((k for k in ("subc", "sub", "mulc", "addc") if c[k]), None) if need_zero else None
        if need_zero and zero_op is None:
            raise ValueError(f"level {l + 1} has AssertZero gates and level {l} no gate that can write a zero row")
        for i in range(c["az"]):  # (first: the zero rows of the previous level are all still there)
            zs = [r for r in self.level_rows[l - 1] if r.alive and r.val == 0]
            if not zs:
                raise ValueError(f"level {l}: no zero row in level {l - 1} for an AssertZero")
            unread = [r for r in zs if r.unread]
            a = unread[0] if unread else zs[i % len(zs)]
            a.unread = False
            self.cov.add(("az", a.kind, "-", "a"))
            self.gate(l, Z64.AssertZero(a.wire), {a.gid})
        for op in ("mul", "add", "sub"):
            for i in range(c[op]):
                self.binary(l, op, i, az_here, zero=(op == zero_op and i < need_zero))
        for op in ("addc", "subc", "mulc"):
            for i in range(c[op]):
                self.unary(l, op, i, az_here, zero=(op == zero_op and i < need_zero))
        self.end_level(l)
        self.table.append(tuple(lv))

    def sink(self):
        left = [r for r in self.rows if r.alive and r.unread]
        if not left:
            return
        n = len(self.level_rows)
        last = [r for r in self.level_rows[n - 1] if r.alive]
        if not last:
            raise ValueError("rows are left unread and the last level writes none for the sink to stand behind")
        tabs = [collections.Counter() for _ in range(3)]
        for _ in range(3):
            self.level_rows.append([])
        zeros = [[], []]
        for k, r in enumerate(left):
            r.unread = False
            if r.level == n - 1:
                w = self.wire()
                zeros[0].append(self.new_row(n, w, 0, "w", self.gate(n, Z64.SubConst(w, r.wire, r.val), {r.gid})))
                tabs[0]["subc"] += 1
            else:
                p = last[k % len(last)]
                w = self.wire()
                t = self.new_row(n, w, r.val - p.val, "w", self.gate(n, Z64.Sub(w, r.wire, p.wire), {r.gid, p.gid}))
                tabs[0]["sub"] += 1
                w = self.wire()
                zeros[1].append(self.new_row(n + 1, w, 0, "w", self.gate(n + 1, Z64.SubConst(w, t.wire, t.val), {t.gid})))
                tabs[1]["subc"] += 1
        for d in (0, 1):
            for z in zeros[d]:
                self.gate(n + 1 + d, Z64.AssertZero(z.wire), {z.gid})
                self.cov.add(("az", "w", "-", "a"))
                tabs[1 + d]["az"] += 1
        for t in tabs:
            if sum(t.values()):
                self.table.append(L(**t))

    # ---- program order
    def emit(self, order, runs):
        n_levels = 1 + max(g[0] for g in self.gates)
        by = [[] for _ in range(n_levels)]
        for gid, g in enumerate(self.gates):
            by[g[0]].append(gid)
        out, done = [], set()

        def put(gid):
            if not self.gates[gid][2] <= done:
                raise ValueError("a gate would stand in front of its operand")
            out.append(gid)
            done.add(gid)

        first = 1
        if runs:
            ins = [g for g in by[0] if self.gates[g][3] is not None]
            muls = [g for g in by[1] if self.gates[g][1][1] == OP_MUL] if n_levels > 1 else []
            if len(ins) != 2 * runs or len(muls) < runs - 1:
                raise ValueError("('runs', k) takes 2 k Inputs on level 0 and at least k - 1 Muls on level 1")
            for g in by[0]:
                if self.gates[g][3] is None:
                    put(g)
            between = set(muls[:runs - 1])
            for j in range(runs):
                put(ins[2 * j])
                put(ins[2 * j + 1])
                if j < runs - 1:
                    put(muls[j])
            for g in by[1]:
                if g not in between:
                    put(g)
            first = 2
        else:
            for g in by[0]:
                put(g)
        l = first
        while l < n_levels:
            if order == "interleaved" and l + 1 < n_levels:
                a, b = collections.deque(by[l]), collections.deque(by[l + 1])
                while a or b:
                    if a:
                        put(a.popleft())
                    if b and (self.gates[b[0]][2] <= done or not a):
                        put(b.popleft())
                l += 2
            else:
                for g in by[l]:
                    put(g)
                l += 1
        ops = [self.gates[g][1] for g in out]
        wit = [self.gates[g][3] for g in out if self.gates[g][3] is not None]
        mul_levels = [self.gates[g][0] for g in out if self.gates[g][1][1] == OP_MUL]
        return ops, wit, mul_levels


Built = collections.namedtuple("Built", "prog wit wc table cov flags mul_levels")


@functools.lru_cache(maxsize=256)
def _build(levels, seed, values, order, inputs):
    if values not in ("random", "edges") or order not in ("by_level", "interleaved"):
        raise ValueError("values: random | edges; order: by_level | interleaved")
    runs = inputs[1] if isinstance(inputs, tuple) else 0
    if not runs and inputs not in ("pairs", "odd"):
        raise ValueError("inputs: pairs | odd | ('runs', k)")
    if runs and order != "by_level":
        raise ValueError("Input runs are placed in the by_level order")
    g = _Gen(seed, values, inplace_ok=(order == "by_level"))
    for l, lv in enumerate(levels):
        need_zero = levels[l + 1][6] if l + 1 < len(levels) else 0  # (that many zero rows, if the level has the gates for them)
        if l == 0:
            g.level0(lv, need_zero, inputs == "odd")
        else:
            g.level(l, lv, need_zero)
    g.sink()
    ops, wit, mul_levels = g.emit(order, runs)
    return Built(program(ops), tuple(wit), (g.n_wires, 0), tuple(g.table), frozenset(g.cov), frozenset(g.flags), tuple(mul_levels))


def _key(levels, seed, values, order, inputs):
    return tuple(tuple(int(x) for x in lv) for lv in levels), seed, values, order, tuple(inputs) if isinstance(inputs, (tuple, list)) else inputs


def class_mix64(levels, seed, values="random", order="by_level", inputs="pairs"):
    """-> (prog, witness, wire_counts); built once per argument tuple and never changed"""
    b = _build(*_key(levels, seed, values, order, inputs))
    return b.prog, list(b.wit), b.wc


def class_table(levels, seed, values="random", order="by_level", inputs="pairs"):
    """the KINDS counts of every level the program compiles to: `levels` as given, then the sink levels (at most three)"""
    return list(_build(*_key(levels, seed, values, order, inputs)).table)


def coverage(levels, seed, values="random", order="by_level", inputs="pairs"):
    """-> (the (op, kind of a, kind of b, form) that occur; flags: sub_wraps, mulc_0, mulc_max)"""
    b = _build(*_key(levels, seed, values, order, inputs))
    return set(b.cov), set(b.flags)


def pre_runs(levels, seed, jw=4, **kw):
    """per level with Mul gates -> (whole wavefront steps of jw Mul gates whose words are consecutive in the preprocessing transcript,
    whole steps where they are not): what k_z64_fused's `pre_run` will see (a Mul's word index is its ordinal among the Muls in
    program order; a level's gates keep their program order)"""
    b = _build(*_key(levels, seed, kw.get("values", "random"), kw.get("order", "by_level"), kw.get("inputs", "pairs")))
    by = collections.defaultdict(list)
    for ep, l in enumerate(b.mul_levels):
        by[l].append(ep)
    out = {}
    for l, eps in sorted(by.items()):
        steps = [eps[i:i + jw] for i in range(0, len(eps) - jw + 1, jw)]
        run = sum(1 for s in steps if s == list(range(s[0], s[0] + jw)))
        out[l] = (run, len(steps) - run)
    return out


# ------------------------------------------------------------------------------------
# the host hooks
# ------------------------------------------------------------------------------------
ELIGIBLE, WHY_GATE, WHY_ODD_M, WHY_RUNS = 0, 1, 2, 3


def fused_levels(prog, wc):
    """rv_hook_z64_fused_levels (host only) -> ([(mul, lin, oth)] per level, eligible: 0, or the reason the circuit is not)"""
    import ctypes as C

    import numpy as np

    from reverie_amd import _lib

    lib = _lib.lib()
    n, why = C.c_size_t(0), C.c_int(-1)
    args = (prog.ctypes.data_as(C.c_void_p), C.c_size_t(len(prog)), C.c_size_t(wc[0]), C.c_size_t(wc[1]), C.c_uint32(0))
    _lib.check(lib.rv_hook_z64_fused_levels(*args, None, C.c_size_t(0), C.byref(n), C.byref(why)))
    out = np.zeros((max(n.value, 1), 4), np.uint32)
    _lib.check(lib.rv_hook_z64_fused_levels(*args, out.ctypes.data_as(C.c_void_p), C.c_size_t(n.value), C.byref(n), C.byref(why)))
    return [(int(r[1] - r[0]), int(r[2] - r[1]), int(r[3] - r[2])) for r in out[:n.value]], why.value


def fused_grid(qw, n_qg, cus, n_mul, n_lin, n_oth):
    """rv_hook_z64_fused_grid (host only) -> (chunks, mul_per, lin_per, oth_per, lin_bias); cus = 0: this machine's"""
    import ctypes as C

    from reverie_amd import _lib

    out = (C.c_uint32 * 5)()
    _lib.check(_lib.lib().rv_hook_z64_fused_grid(qw, n_qg, cus, n_mul, n_lin, n_oth, out))
    return tuple(int(x) for x in out)


def machine_cus():
    """the compute units the fused launcher plans for here (256 where no device answers): read back from the grid hook, whose chunk
    count for a level of Mul gates alone is min(cus, ceil(n_mul / 32)) at one quad group of 16"""
    return fused_grid(16, 1, 0, 1 << 20, 0, 0)[0]


# ------------------------------------------------------------------------------------
# Labels.  Plain transcriptions of the launcher's and the kernel's arithmetic that NAME the split a spec hits, so that the host test
# can assert the specs cover what the GPU file says they cover.  They are labels, not oracles: nothing is computed from them that a
# proof is compared with -- the oracle's proof is the only reference.
# ------------------------------------------------------------------------------------
def wave_plan(n_m, n_l, jw, lin_bias=LIN_BIAS):
    """A transcription of k_z64_fused's x, MI, LI and l0s for a workgroup with n_m Mul and n_l linear gates in wavefront steps of jw.
    A label, not an oracle: it names the regime ("plenty": ql_ > lin_bias, "equal", "scarce") and the residue x = TM % 8 a spec
    hits; no test derives an expected proof byte from it."""
    tm, tl = -(-n_m // jw), -(-n_l // jw)
    x = tm % 8
    ql = (tl + lin_bias * x + 7) // 8
    regime = "plenty" if ql > lin_bias else "equal" if ql == lin_bias else "scarce"
    if ql < lin_bias:
        ql = -(-tl // (8 - x))
    qh = ql - lin_bias if ql > lin_bias else 0
    mi = [tm // 8 + (1 if w < x else 0) for w in range(8)]
    li = [qh if w < x else ql for w in range(8)]
    l0s = [w * qh if w < x else x * qh + (w - x) * ql for w in range(8)]
    return {"TM": tm, "TL": tl, "x": x, "regime": regime, "MI": mi, "LI": li, "l0s": l0s,
            "tail_only": any(m == 0 and n > 0 for m, n in zip(mi, li)), "rem": (n_m % jw, n_l % jw)}


def chunk_counts(counts, grid):
    """[(n_m, n_l, n_o)] of every workgroup chunk of a level of counts = (mul, lin, oth) under grid = fused_grid(...)"""
    chunks, per = grid[0], grid[1:4]
    return [tuple(max(0, min(n - c * p, p)) for n, p in zip(counts, per)) for c in range(chunks)]


def level_labels(counts, qw, n_qg, cus):
    """-> (the grid branches a level of counts = (mul, lin, oth) takes, {(regime, x, tail_only)} over its chunks with Mul or linear
    gates, {(class, remainder)} of the chunks' last steps)"""
    jw = 64 // qw
    step = 8 * jw
    n_mul, n_lin, n_oth = counts
    grid = fused_grid(qw, n_qg, cus, *counts)
    chunks = grid[0]
    if not chunks:
        return {"empty"}, set(), set()
    per_qg = max(cus // n_qg, 1)
    mul_chunks = min(per_qg, -(-n_mul // step)) if n_mul else 1
    mem_chunks = min(-(-(n_lin + n_oth) // (2 * step)), per_qg * (1 if n_mul else 4))
    assert chunks == max(mul_chunks, mem_chunks, 1)
    br = set()
    if chunks == 1:
        br.add("one-chunk")
    if chunks == 2:
        br.add("two-chunks")
    if n_mul and -(-n_mul // step) > per_qg and chunks == per_qg:
        br.add("saturated")
    if n_mul and -(-n_mul // step) == per_qg and chunks == per_qg:
        br.add("at-per_qg")
    if n_mul and mem_chunks > mul_chunks:
        br.add("mem>mul")
    if not n_mul and chunks > per_qg:
        br.add("no-mul-allowance")
    if any(n and (chunks - 1) * p >= n for n, p in zip(counts, grid[1:4])):
        br.add("trailing-empty")
    deal, rem = set(), set()
    for n_m, n_l, n_o in chunk_counts(counts, grid):
        if n_m or n_l:
            wp = wave_plan(n_m, n_l, jw, grid[4])
            deal.add((wp["regime"], wp["x"], wp["tail_only"]))
        for cls, n, unit in (("mul", n_m, jw), ("lin", n_l, jw), ("oth", n_o, step)):
            if n:
                rem.add((cls, n % unit))
    return br, deal, rem


# ------------------------------------------------------------------------------------
# The specs of test_gpu_level_classes64.py, each pinned by test_class_mix64_host.py.  JW = 64 / QW gates per wavefront step and
# STEP = 8 JW per workgroup step: 4 and 32 at QW = 16 (whole proofs, shards of 128 and 64 repetitions), 8 and 64 at QW = 8 (shards of
# 32).  A level's linear gates are spread over the five ops by lin().
# ------------------------------------------------------------------------------------
SEED = 11


def lin(n, az=0, mul=0):
    """a level of `mul` Mul gates, n linear gates over the five ops (SubConst first: it writes the zero row of an AssertZero behind) and
    `az` AssertZero gates"""
    q, r = divmod(n, 5)
    c = [q + (1 if i < r else 0) for i in range(5)]
    return L(mul=mul, subc=c[0], add=c[1], sub=c[2], mulc=c[3], addc=c[4], az=az)


def inputs0(n=16, const=4):
    return L(inp=n, const=const)


def deal_spec(n_mul, n_lin):
    """one level of n_mul Mul and n_lin linear gates behind 16 Inputs and 4 Consts, a level of 8 linear gates in front of it (so its
    operands are mask rows and wmask rows) and a level of 5 behind it; the sink reads the rest"""
    return [inputs0(), lin(8, mul=4), lin(n_lin, mul=n_mul) if n_lin else L(mul=n_mul), lin(5)]


# The wavefront deal.  ql_ = (TL + 3 x + 7) // 8 against lin_bias = 3 gives "plenty" from TL = 25 - 3 x, "equal" from 17 - 3 x and
# "scarce" below (none for x = 6, 7: 3 x + 7 >= 24, so ql_ >= 3 with no linear step at all).  While the chunk count is not saturated
# a chunk holds at most 8 Mul steps and 16 linear ones, so in a level of ONE chunk x = TM % 8 is TM itself (the wavefronts from x on
# run no Mul step and all their linear steps in the tail loop) and "plenty" begins at x = 3, "equal" at x = 1; (regime, x) -> the
# smallest (n_mul, n_lin) with one chunk, remainders of 1 where there is a choice, at JW = 4 and at JW = 8:
DEAL_ONE_CHUNK = {
    4: {("equal", 1): (1, 53), ("equal", 2): (5, 41), ("equal", 3): (9, 29), ("equal", 4): (13, 17), ("equal", 5): (17, 5), ("equal", 6): (21, 1),
        ("equal", 7): (25, 1), ("plenty", 3): (9, 61), ("plenty", 4): (13, 49), ("plenty", 5): (17, 37), ("plenty", 6): (21, 25),
        ("plenty", 7): (25, 13), ("scarce", 0): (29, 1), ("scarce", 1): (1, 1), ("scarce", 2): (5, 1), ("scarce", 3): (9, 1), ("scarce", 4): (13, 1),
        ("scarce", 5): (17, 1)},
    8: {("equal", 1): (1, 105), ("equal", 2): (9, 81), ("equal", 3): (17, 57), ("equal", 4): (25, 33), ("equal", 5): (33, 9), ("equal", 6): (41, 1),
        ("equal", 7): (49, 1), ("plenty", 3): (17, 121), ("plenty", 4): (25, 97), ("plenty", 5): (33, 73), ("plenty", 6): (41, 49),
        ("plenty", 7): (49, 25), ("scarce", 0): (57, 1), ("scarce", 1): (1, 1), ("scarce", 2): (9, 1), ("scarce", 3): (17, 1), ("scarce", 4): (25, 1),
        ("scarce", 5): (33, 1)},
}
# ... plus TL = 0 (no linear gate: every LI is 0) beside 5 and beside 8 JW Mul gates
DEAL_NO_LIN = {4: [(5, 0), (32, 0)], 8: [(9, 0), (64, 0)]}
DEAL_REGIMES = [(r, x) for x in range(8) for r in ("plenty", "equal", "scarce") if r != "scarce" or x < 6]


def deal_sat_specs(cus, qw=16, n_qg=4):
    """(regime, x) -> (n_mul, n_lin) for every regime there is, with the chunk count saturated at per_qg = cus / n_qg so that every
    chunk holds 8 + x Mul steps (every wavefront runs the main loop, x of them twice) and TL linear steps: the deal of the benchmark's
    levels.  The last chunk is one gate short in either class."""
    jw = 64 // qw
    per_qg = max(cus // n_qg, 1)
    out = {}
    for reg, x in DEAL_REGIMES:
        tl = {"plenty": 26 - 3 * x, "equal": max(17 - 3 * x, 0) + 3, "scarce": 1 if x == 5 else 2}[reg]
        out[(reg, x)] = (per_qg * jw * (8 + x) - 1, per_qg * jw * tl - 1)
    return out


# levels whose chunks hold more than one round of Mul steps (TM >= 8 in a chunk) exist only with the chunk count saturated at per_qg:
# chunk_specs(cus) below builds them from the machine's compute units
def chunk_specs(cus, qw=16, n_qg=4):
    """name -> (levels, index of the level under test, the grid branch it is named for), for `cus` compute units"""
    jw = 64 // qw
    step = 8 * jw
    per_qg = max(cus // n_qg, 1)

    def one(n_mul, n_lin=0, n_oth=0):
        # n_oth AssertZero gates read one zero row; a level of linear gates in front gives both kinds of operand rows
        mix = lin(n_lin, az=n_oth, mul=n_mul) if n_lin else L(mul=n_mul, az=n_oth)
        return [inputs0(), lin(8 if not n_oth else 10, mul=4), mix], 2

    return {
        "mul-step": one(step) + ("one-chunk",),
        "mul-step+1": one(step + 1) + ("two-chunks",),
        "mul-per_qg": one(step * per_qg) + ("at-per_qg",),
        "mul-per_qg+1": one(step * per_qg + 1) + ("saturated",),
        "one-mul-beside-lin": one(1, 4 * step + 1) + ("mem>mul",),
        "one-mul-beside-lin-trailing": one(1, 4 * step + 1) + ("trailing-empty",),
        "no-mul": one(0, 2 * step * per_qg + 1) + ("no-mul-allowance",),
        "oth-two-chunks": one(0, 5, 2 * step + 1) + ("two-chunks",),
    }


def rem_specs(jw):
    """step remainders: n_mul, n_lin at 1 and -1 mod JW, n_oth at 1 and -1 mod STEP, each beside a few gates of the others"""
    step = 8 * jw
    out = {}
    for r, tag in ((1, "+1"), (-1, "-1")):
        out["mul" + tag] = [inputs0(), lin(8, mul=4), lin(5, mul=2 * jw + r), lin(5)]
        out["lin" + tag] = [inputs0(), lin(8, mul=4), lin(2 * jw + r, mul=3), lin(5)]
        out["oth" + tag] = [inputs0(), lin(10, mul=4), lin(5, az=step + r, mul=3)]
    return out


SINGLE_SPECS = {
    "only-mul": [inputs0(), L(mul=9)],
    "only-add": [inputs0(), L(add=9)],
    "only-sub": [inputs0(), L(sub=9)],
    "only-addc": [inputs0(), L(addc=9)],
    "only-subc": [inputs0(), L(subc=9)],
    "only-mulc": [inputs0(), L(mulc=9)],
    "only-az": [L(inp=8), L(subc=8), L(az=8)],
    "inputs-only": [L(inp=10)],
    "consts-only": [L(const=5)],
    "inputs-and-consts": [L(inp=6, const=3)],
}
MIXED = [inputs0(34, 5), lin(23, mul=13), lin(31, az=3, mul=37), lin(9, mul=5), lin(12, az=2, mul=6), lin(7, mul=3)]
_ROT = L(mul=40, add=20, sub=20, addc=6, subc=6, mulc=6)
ROTATION = [inputs0(20, 6), _ROT, _ROT, L(mul=20, add=20, sub=20, addc=6, subc=6, mulc=6, az=2), lin(10, mul=4)]
INTERLEAVED = [inputs0(40, 4), lin(20, mul=24), lin(20, mul=24), lin(10, mul=16), lin(10, mul=16)]
ODD_INPUTS = [L(inp=7, const=2), lin(6, mul=5), lin(5, mul=4)]


def runs_spec(k):
    return [L(inp=2 * k), lin(6, mul=k + 2), lin(5, mul=3)]


WIDE_LIN = [inputs0(), lin(2100), lin(40)]              # a level of more than 2 048 gates: k_interp64's grid cap
BATCH_SMALL = [inputs0(), lin(9, mul=7), lin(6, az=2, mul=5)]
BATCH_WIDE = [inputs0(), lin(700, mul=3), lin(30, mul=2)]  # more than 8 192 / 4 / 3 = 682 workers per proof in a batch of three
# the forms test_class_mix64_host.py asks of ROTATION: both operand kinds on either side of every two-operand op, every form
WANT_FORMS = {(op, ka, kb, "ab") for op in ("mul", "add", "sub") for ka in "mw" for kb in "mw"}
WANT_FORMS |= {(op, k, k, "same") for op in ("mul", "add", "sub") for k in "mw"}
WANT_FORMS |= {(op, ka, kb, f) for op in ("mul", "add", "sub") for f in ("ba", "dst_a", "dst_b") for ka, kb in (("m", "w"), ("w", "m"))}
WANT_FORMS |= {(op, k, "-", f) for op in ("addc", "subc", "mulc") for k in "mw" for f in ("a", "dst_a")}
WANT_FORMS |= {("az", "w", "-", "a")}


# ------------------------------------------------------------------------------------
# Every spec of test_gpu_level_classes64.py in one table (test_class_mix64_host.py pins each of them, the GPU file runs exactly these)
# ------------------------------------------------------------------------------------
Spec = collections.namedtuple("Spec", "name levels kw why at")  # kw: class_mix64's options; why: ELIGIBLE or the reason; at: the level under test or None
SPLIT64_MULS = 4351  # the fewest Mul gates behind inputs0() whose proof has 4 MiB of online records (the verifier's side copy, split64)


def all_specs(cus):
    """name -> Spec, for a machine of `cus` compute units (the chunk-edge and saturated-deal specs are sized by it)"""
    out = {}

    def add(name, levels, why=ELIGIBLE, at=None, **kw):
        assert name not in out
        out[name] = Spec(name, levels, kw, why, at)

    for jw in (4, 8):
        for (reg, x), (m, n) in DEAL_ONE_CHUNK[jw].items():
            add(f"deal{jw}-{reg}-{x}", deal_spec(m, n), at=2)
        for m, n in DEAL_NO_LIN[jw]:
            add(f"deal{jw}-nolin-{m}", deal_spec(m, n), at=2)
        for name, lv in rem_specs(jw).items():
            add(f"rem{jw}-{name}", lv, at=2)
    for (reg, x), (m, n) in deal_sat_specs(cus).items():
        add(f"sat-{reg}-{x}", deal_spec(m, n), at=2)
    for name, (lv, at, _) in chunk_specs(cus).items():
        add("chunk-" + name, lv, at=at)
    for name, lv in SINGLE_SPECS.items():
        add(name, lv)
    add("mixed", MIXED)
    add("mixed-edges", MIXED, values="edges")
    add("rotation", ROTATION)
    add("rotation-edges", ROTATION, values="edges")
    add("interleaved", INTERLEAVED, order="interleaved")
    add("odd-inputs", ODD_INPUTS, why=WHY_ODD_M, inputs="odd")
    add("runs-64", runs_spec(64), inputs=("runs", 64))
    add("runs-65", runs_spec(65), why=WHY_RUNS, inputs=("runs", 65))
    add("wide-lin", WIDE_LIN, at=1)
    add("batch-small", BATCH_SMALL)
    add("batch-wide", BATCH_WIDE, at=1)
    add("split64", [inputs0(), L(mul=SPLIT64_MULS)], at=1)
    return out


def build(spec):
    """-> (prog, witness, wire_counts, [(mul, lin, oth)] per level with the sink)"""
    prog, wit, wc = class_mix64(spec.levels, SEED, **spec.kw)
    return prog, wit, wc, [bounds(t) for t in class_table(spec.levels, SEED, **spec.kw)]
