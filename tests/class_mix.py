"""GF(2) programs whose compiled levels hold a chosen number of gates of every class (csrc/internal.h: LevelRange), for the tests
that aim at one level executor at a time: test_class_mix_host.py proves on the host compiler alone that every spec compiles to
exactly its class counts and run plan, test_gpu_level_classes.py runs the same specs against the oracle.

class_mix(levels, seed) -> (prog, witness, wire_counts); the program is meant for the lazy-sum form (Circuit(..., whole_prover=True)).
levels[l] = (c0, c1, c2, c3, c4) or (c0, c1, c2, c3, c4, options): the gates of dependency level l by class --

  0  Mul of two row wires (one base row per operand; either may carry a constant)
  1  Mul with another operand shape: operands of na, nb in 0 .. 3 base rows (0: a pure constant) other than (1, 1), with and
     without the operands' constants
  2  a materialised sum of two rows, with and without the constant
  3  a materialised sum of 3 rows, or of 4, 5, 6 rows (na = 3, nb = 1 .. 3), with and without the constant
  4  level 0: Input (and options["random"] Random) ops; later levels: AssertZero of a form of 1 .. 3 rows plus its clear value

The construction rests on the compiler's materialisation rule (tests/lazy_corpus.py): a sum of n rows read f times stays symbolic
when n <= 1, or n <= 3 and f (n - 1) <= n + 1.  A sum that feeds one Mul or AssertZero is read once and stays symbolic; a sum that is
to become a gate gets four more reads from two dead ops Add(dump, s, s) -- a read by a dead sum counts, and a dead sum is dropped, so
forcing a row costs no gate in any level.  A gate sits on the level behind its latest base row, so every gate of level l takes one
row written by level l - 1 and the rest from any earlier level.

Every row a gate writes is read again by a live gate of a later level -- a gate whose result nothing reads could compute anything --
taking rows nobody has read yet first.  What is still unread after the last level is read by a sink level of AssertZero gates that
the generator appends (one row of the last level and up to two others per gate); class_table() reports the levels with that sink.
A Random op's row differs between the repetitions, so no assertion may depend on it: it is the second operand of the first class-0
Mul of the last level (whose result is then left unread), or unread when that level has none.

Level 0 holds what depends on no row: c0 = c2 = c3 = 0 there, and its c1 are Muls of two constants (na = nb = 0)."""
import collections
import functools
import random

from reverie_amd.ops import GF2, program

# class 1: (na, nb) other than (1, 1) and, behind level 0, (0, 0); every pair with the four (ca, cb)
_MUL_SHAPES = [(na, nb, ca, cb) for ca in (0, 1) for cb in (0, 1) for na in range(4) for nb in range(4) if (na, nb) not in ((1, 1), (0, 0))]
_XOR3_SHAPES = [(n, c) for c in (0, 1) for n in (3, 4, 5, 6)]


def _norm(levels):
    out = []
    for lv in levels:
        opts = dict(lv[5]) if len(lv) > 5 else {}
        out.append(tuple(int(x) for x in lv[:5]) + (tuple(sorted(opts.items())),))
    return tuple(out)


class _Gen:
    def __init__(self, seed):
        self.rng = random.Random(seed)
        self.ops = []
        self.wit = []
        self.val = [0]          # clear value per wire; wire 0 is the dump wire of the dead ops
        self.by_level = []      # row wires (one base row, no constant) written by each level
        self.avail = []         # row wires of every finished level
        self.unread = collections.deque()
        self.is_unread = set()
        self.fresh_at = 0       # round-robin position in the previous level's rows
        self.prev_unread = collections.deque()  # rows of the previous level nobody has read yet
        self.table = []

    def wire(self, v):
        self.val.append(v & 1)
        return len(self.val) - 1

    # ---- operand choice
    def mark(self, w):
        self.is_unread.discard(w)

    def fresh(self, l):
        prev = self.by_level[l - 1]
        if not prev:
            raise ValueError(f"level {l}: level {l - 1} writes no row for its gates to stand behind")
        while self.prev_unread:  # an unread row of the previous level first
            w = self.prev_unread.popleft()
            if w in self.is_unread:
                return w
        w = prev[self.fresh_at % len(prev)]
        self.fresh_at += 1
        return w

    def older(self, taken):
        while self.unread:
            w = self.unread[0]
            if w not in self.is_unread:
                self.unread.popleft()
                continue
            if w in taken:
                break
            return w
        if len(self.avail) <= len(taken):
            raise ValueError("too few rows for a sum of distinct rows: widen the levels below")
        while True:
            w = self.avail[self.rng.randrange(len(self.avail))]
            if w not in taken:
                return w

    def rows(self, l, n):
        """n distinct row wires of levels < l, the first one of level l - 1"""
        if n == 0:
            return []
        got = [self.fresh(l)]
        while len(got) < n:
            got.append(self.older(got))
        for w in got:
            self.mark(w)
        return got

    # ---- building blocks
    def form(self, rows, c):
        """a wire holding XOR(rows) ^ c through sums that are read once -> wire"""
        if not rows:
            w = self.wire(c)
            self.ops.append(GF2.Const(w, c))
            return w
        cur = rows[0]
        for r in rows[1:]:
            w = self.wire(self.val[cur] ^ self.val[r])
            self.ops.append(GF2.Add(w, cur, r))
            cur = w
        if c:
            w = self.wire(self.val[cur] ^ 1)
            self.ops.append(GF2.AddConst(w, cur, 1))
            cur = w
        return cur

    def new_row(self, l, w):
        self.by_level[l].append(w)

    def end_level(self, l):
        """the level's rows become operands of the levels behind it"""
        self.avail += self.by_level[l]
        self.prev_unread = collections.deque()
        for w in self.by_level[l]:
            if l == 0 and w in self.inputs:
                continue  # (an Input gate writes its transcript row itself: nothing has to read it)
            self.unread.append(w)
            self.is_unread.add(w)
            self.prev_unread.append(w)

    def mul(self, l, a, b, tainted=False):
        w = self.wire(self.val[a] & self.val[b])
        self.ops.append(GF2.Mul(w, a, b))
        if not tainted:
            self.new_row(l, w)

    def xork(self, l, n, c):
        rows = self.rows(l, n)
        if n <= 3:
            s = self.form(rows[:1], c)
            for r in rows[1:]:
                w = self.wire(self.val[s] ^ self.val[r])
                self.ops.append(GF2.Add(w, s, r))
                s = w
        else:
            a, b = self.form(rows[:3], c), self.form(rows[3:], 0)
            s = self.wire(self.val[a] ^ self.val[b])
            self.ops.append(GF2.Add(s, a, b))
        self.ops += [GF2.Add(0, s, s), GF2.Add(0, s, s)]  # four reads by dead sums: the sum becomes a row
        self.new_row(l, s)

    def assert_rows(self, rows):
        v = 0
        for r in rows:
            v ^= self.val[r]
        self.ops.append(GF2.AssertZero(self.form(rows, v)))

    # ---- levels
    def level0(self, c, opts):
        c0, c1, c2, c3, c4 = c
        n_rand = int(opts.get("random", 0))
        if c0 or c2 or c3 or n_rand > c4:
            raise ValueError("level 0 holds Input, Random and constant Mul gates only")
        self.by_level.append([])
        self.randoms = []
        self.inputs = set()
        for i in range(c4):
            if i >= c4 - n_rand:
                w = self.wire(0)
                self.ops.append(GF2.Random(w))
                self.randoms.append(w)
            else:
                bit = self.rng.randrange(2)
                w = self.wire(bit)
                self.ops.append(GF2.Input(w))
                self.wit.append(bit)
                self.by_level[0].append(w)
                self.inputs.add(w)
        for i in range(c1):
            a, b = self.form([], i & 1), self.form([], (i >> 1) & 1)
            self.mul(0, a, b)

    def level(self, l, c, last):
        c0, c1, c2, c3, c4 = c
        self.by_level.append([])
        self.fresh_at = 0
        for i in range(c0):
            tainted = last and i == 0 and bool(self.randoms)
            if tainted:
                x, y = self.rows(l, 1)[0], self.randoms[0]
            else:
                x, y = self.rows(l, 2)
            self.mul(l, self.form([x], i & 1), self.form([y], (i >> 1) & 1 if not tainted else 0), tainted)
        for i in range(c1):
            na, nb, ca, cb = _MUL_SHAPES[(i * 5 + l) % len(_MUL_SHAPES)]  # (5 and 56 are coprime: every shape in turn)
            rows = self.rows(l, na + nb)
            if self.rng.randrange(2) and na and nb:  # the row of the previous level in either operand
                rows = rows[1:] + rows[:1]
            self.mul(l, self.form(rows[:na], ca), self.form(rows[na:], cb))
        for i in range(c2):
            self.xork(l, 2, (i + l) & 1)
        for i in range(c3):
            n, cc = _XOR3_SHAPES[(i * 3 + l) % len(_XOR3_SHAPES)]
            self.xork(l, n, cc)
        for i in range(c4):
            self.assert_rows(self.rows(l, 1 + (i + l) % 3))

    def sink(self):
        left = [w for w in self.unread if w in self.is_unread]
        if not left:
            return
        l = len(self.by_level)
        last = self.by_level[-1]
        if not last:
            raise ValueError("rows are left unread and the last level writes none for a sink level to stand behind")
        in_last = set(last)
        head = [w for w in left if w in in_last]
        rest = [w for w in left if w not in in_last]
        n = 0
        k = 0
        while head or rest:
            first = head.pop() if head else last[k % len(last)]
            k += 1
            more = []
            while len(more) < 2 and (rest or len(head) > 0):
                more.append(rest.pop() if rest else head.pop())
            self.assert_rows([first] + more)
            n += 1
        self.is_unread.clear()
        self.table.append((0, 0, 0, 0, n))


@functools.lru_cache(maxsize=64)
def _build(levels, seed):
    g = _Gen(seed)
    for l, lv in enumerate(levels):
        c, opts = lv[:5], dict(lv[5])
        if l == 0:
            g.level0(c, opts)
        else:
            if opts:
                raise ValueError("options belong to level 0")  # random: Random ops among its c4; sink: 0 leaves the last level's rows unread
            g.level(l, c, l == len(levels) - 1)
        g.end_level(l)
        g.table.append(c)
    if dict(levels[0][5]).get("sink", 1):
        g.sink()
    return program(g.ops), g.wit, (0, len(g.val)), tuple(g.table)


def class_mix(levels, seed):
    """-> (prog, witness, wire_counts); built once per (levels, seed) and never changed"""
    prog, wit, wc, _ = _build(_norm(levels), seed)
    return prog, list(wit), wc


def class_table(levels, seed):
    """the (c0, c1, c2, c3, c4) of every level the program compiles to: `levels` as given, then the sink level if there is one"""
    return list(_build(_norm(levels), seed)[3])


def level_table(prog, wc, whole_prover=True):
    """rv_hook_compile_levels (host only) -> [(c0, c1, c2, c3, c4, has_z64, run, tiny)] per compiled level"""
    import ctypes as C

    import numpy as np

    from reverie_amd import _lib

    L = _lib.lib()
    n = C.c_size_t(0)
    args = (prog.ctypes.data_as(C.c_void_p), C.c_size_t(len(prog)), C.c_size_t(wc[0]), C.c_size_t(wc[1]), C.c_uint32(1 if whole_prover else 0))
    _lib.check(L.rv_hook_compile_levels(*args, None, C.c_size_t(0), C.byref(n)))
    out = np.zeros((n.value, 10), np.int32)
    _lib.check(L.rv_hook_compile_levels(*args, out.ctypes.data_as(C.c_void_p), C.c_size_t(n.value), C.byref(n)))
    return [tuple(int(x) for x in (r[1] - r[0], r[2] - r[1], r[3] - r[2], r[4] - r[3], r[5] - r[4], r[6], r[7], r[8])) for r in out]


# ------------------------------------------------------------------------------------
# The specs of test_gpu_level_classes.py, each pinned by test_class_mix_host.py.  Level 0 is 300 Inputs wherever the levels behind it
# are to be launched on their own: a narrow run needs three consecutive levels of at most 256 gates, and behind a wide level 0
# there are two (the mix and the sink).
# ------------------------------------------------------------------------------------
def wide0(rand=0, n=300):
    return (0, 0, 0, 0, n, {"random": 1}) if rand else (0, 0, 0, 0, n)


# class counts around every step of the class loops: 4 gates at 64 quad words per row, 8 at 32 and 16, 16 at 8
STEP_COUNTS = sorted({c for s in (4, 8, 16) for c in (0, 1, s - 1, s, s + 1, 2 * s + 1)})


def step_mix(kind, cls, n):
    """level 1 of a step-remainder circuit: class `cls` holds n gates; kind "fast": the others 3 each (c1 + c3 < 64), "alone": the
    others empty, "general": c1 + c3 >= 64 through the other multi-base class"""
    c = [0] * 5 if kind == "alone" else [3] * 5
    if kind == "general":
        c[1], c[3] = (64, 40) if cls == 3 else (40, 64) if cls == 1 else (40, 40)
    c[cls] = n
    return tuple(c)


def step_specs(kind, cls, rand):
    """-> [(name, levels)] of one (kind, class) cell of the step-remainder matrix"""
    counts = [n for n in STEP_COUNTS if n or kind != "alone"]
    return [(f"{kind}-c{cls}-{n}", [wide0(rand), step_mix(kind, cls, n)]) for n in counts]


# 1 to 5 gates over three classes: the wavefront of a class's first step rotates with the classes in front of it (run_level's `slot`)
SLOT_SPECS = [("slot-%d" % i, [wide0(r), m]) for r in (0, 1) for i, m in enumerate([(1, 1, 1, 0, 0), (0, 1, 0, 1, 1), (2, 0, 1, 0, 2), (0, 2, 2, 0, 1), (1, 0, 0, 2, 1)])]

# the switch to the kernel variant with the multi-base loops, c1 + c3 at 63 / 64 / 65
GENERAL_SWITCH = [(63, 0), (0, 63), (64, 0), (0, 64), (32, 33)]


def switch_own(c1, c3, rand):
    return [wide0(rand), (120, c1, 60, c3, 300 - 180 - c1 - c3)]  # 300 gates: a launch of its own


def switch_in_run(c1, c3):
    """eight levels wider than 32 gates behind a wide level 0: a class-loop run, not lean; the switch level in its middle"""
    lv = [(16, 1, 10, 1, 8)] * 4 + [(40, c1, 30, c3, 20)] + [(16, 1, 10, 1, 8)] * 2 + [(30, 1, 30, 1, 60)]
    return [wide0(1)] + lv


def narrow_levels(n_levels, rand=0):
    """a wide level 0 and n_levels - 1 levels of 12 gates behind it (the sink is the n_levels-th narrow level)"""
    return [wide0(rand)] + [(4, 2, 2, 2, 2)] * (n_levels - 1)


_WIDE = (10, 0, 0, 0, 290)  # a separator of 300 gates that reads what the levels in front of it left unread
_N33, _N32, _N20, _N40 = (12, 3, 8, 2, 8), (12, 3, 8, 1, 8), (8, 2, 4, 2, 4), (14, 3, 10, 3, 10)
_LEAN = (20, 0, 12, 0, 8)
WINDOW_WIDTHS = [200, 256, 230, 210, 256, 201, 249, 222, 256, 200]


def _w(n):  # a level of n gates, every class present
    return (n - 4 * (n // 5), n // 5 - 20, n // 5, 20, 2 * (n // 5))


# name -> (levels, expected narrow runs [(first level, end, tiny)]): every other level is launched on its own
RUN_SPECS = {
    "two-then-three": ([wide0(1), _N20, _N20, _WIDE, _N20, _N20, _N20, _WIDE], [(4, 7, 1)]),
    "7x33-8x33-8x32": ([wide0(1)] + [_N33] * 7 + [_WIDE] + [_N33] * 8 + [_WIDE] + [_N32] * 8 + [_WIDE], [(1, 8, 1), (9, 17, 0), (18, 26, 1)]),
    "256": ([wide0(1), _N20, _w(256), _N20], [(1, 5, 1)]),
    "257": ([wide0(1), _N20, _w(257), _N20], []),
    "merge": ([wide0(1)] + [_N20] * 3 + [_N40] * 3 + [_N20] * 3, [(1, 11, 1)]),
    "lean": ([wide0(1)] + [_LEAN] * 7 + [(20, 0, 12, 0, 120)], [(1, 9, 2), (9, 10, 1)]),
    "not-lean": ([wide0(1)] + [_LEAN] * 3 + [(20, 1, 12, 0, 7)] + [_LEAN] * 3 + [(20, 0, 12, 0, 120)], [(1, 9, 0), (9, 10, 1)]),
    "window": ([wide0(1)] + [_w(n) for n in WINDOW_WIDTHS[:-1]] + [(60, 20, 40, 20, 60)], [(1, 12, 0)]),
    "1025": ([wide0()] + [_N33] * 1023 + [(100, 0, 0, 0, 0)], [(1, 1026, 0)]),
}
VCLR_SPECS = {16: narrow_levels(16), 17: narrow_levels(17)}

GRID_SPECS = {
    "cap-fast": [wide0(0, 4096), (40000, 30, 20000, 30, 9940)],
    "cap-general": [wide0(0, 4096), (30000, 10000, 15000, 10000, 5000)],
    "prefetch-tiny-next": [wide0(0, 4096), (10000, 20, 8000, 20, 1960), (1, 0, 0, 0, 0)],
    "prefetch-no-next": [(0, 0, 0, 0, 4096, {"sink": 0}), (12000, 30, 0, 0, 7970)],
}
BATCH_OWN = [wide0(), (5, 6, 7, 9, 3)]
BATCH_RUN = [wide0()] + [_N33] * 4 + [_N20] * 3 + [_N40] * 9
