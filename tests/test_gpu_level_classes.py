"""Every GF(2) level executor against the oracle, level by gate-class mix.  tests/class_mix.py builds programs whose compiled levels
hold a chosen number of gates of each class (test_class_mix_host.py pins that on the host); here each of them is proved and verified
on the GPU -- the proof byte for byte the oracle's, the strict verifier accepting it, a proof with a flipped broadcast or correction
byte answered as the oracle answers it -- and rv_hook_interp_launches must show, around every call, exactly the launches that the
circuit's plan (rv_hook_circuit_levels) predicts for the executor the case is for and none of any other."""
import collections
import ctypes as C
import struct

import numpy as np
import pytest

import class_mix as cm

pytestmark = pytest.mark.gpu

ROWS = ["full_fast", "full_general", "generic", "narrow_gate", "narrow_class", "narrow_lean", "lds", "b_full", "b_narrow_gate", "b_narrow_class", "b_lds"]
P, PV, V, VC = 0, 1, 2, 3  # the counters' columns: MODE_PROVE, MODE_PROVE_V, MODE_VERIFY, MODE_VERIFY_C
SEED = 7  # (the seed test_class_mix_host.py pins the specs with)
CLASS_NQ = (64, 32, 16, 8)  # row widths with a k_interp_full / class-loop instantiation


@pytest.fixture(scope="module")
def rv():
    import reverie_amd

    reverie_amd.Context.default()
    return reverie_amd


@pytest.fixture(autouse=True)
def _plain_env(monkeypatch):
    for k in ("RV_LDS_RUN", "RV_LDS_QS", "RV_LDS_BATCH_WGS", "RV_VERIFY_VC"):
        monkeypatch.delenv(k, raising=False)


def launches():
    """the launches since the last call -> {(executor, mode column): count}"""
    from reverie_amd import _lib

    counts = ((C.c_uint64 * 4) * len(ROWS))()
    _lib.check(_lib.lib().rv_hook_interp_launches(counts, C.c_int(1)))
    return {(ROWS[e], m): int(counts[e][m]) for e in range(len(ROWS)) for m in range(4) if counts[e][m]}


def circuit_levels(c):
    """rv_hook_circuit_levels -> ([levels][10] table, vclr_ok, general_levels)"""
    from reverie_amd import _lib

    L = _lib.lib()
    n, vclr, gen = C.c_size_t(0), C.c_int(-1), C.c_int(-1)
    _lib.check(L.rv_hook_circuit_levels(c.handle, None, C.c_size_t(0), C.byref(n), None, None))
    out = np.zeros((n.value, 10), np.int32)
    _lib.check(L.rv_hook_circuit_levels(c.handle, out.ctypes.data_as(C.c_void_p), C.c_size_t(n.value), C.byref(n), C.byref(vclr), C.byref(gen)))
    return out, bool(vclr.value), bool(gen.value)


def predict(table, nq, mode):
    """the launches of one pass over the levels at rows of nq quad words (csrc/shard.inc: shard_run_levels)"""
    out = collections.Counter()
    own = mode in (PV, VC)  # (these modes exist in the one-launch-per-level kernels only)
    pv = V if mode in (V, VC) else P  # the column of the kernels that exist as PROVE and VERIFY only
    run_len = collections.Counter(int(r[7]) for r in table if r[7] >= 0)
    prev_run = prev_lds = -1
    for r in table:
        c1, c3, width, run, tiny, lds = r[2] - r[1], r[4] - r[3], r[5] - r[0], int(r[7]), int(r[8]), int(r[9])
        if not own and lds >= 0 and nq % 8 == 0:  # (one-quad slices need rows of whole 32-bit corr words: lds_run_fits_rows)
            out[("lds", pv)] += lds != prev_lds
            prev_lds = lds
        elif not own and run >= 0:
            if run != prev_run:
                kernel = "narrow_gate" if tiny == 1 or nq not in CLASS_NQ else "narrow_lean" if tiny == 2 and nq == 64 else "narrow_class"
                out[(kernel, pv)] += (run_len[run] + 1023) // 1024
            prev_run = run
        elif width and nq in CLASS_NQ:
            out[("full_general" if c1 + c3 >= 64 else "full_fast", mode if nq == 64 or mode != VC else V)] += 1
        elif width:
            out[("generic", pv)] += 1
    return {k: v for k, v in out.items() if v}


def predict_batch(table, batch, mode, lds_limit):
    """csrc/batch.inc: launch_levels_batched"""
    out = collections.Counter()
    run_len = collections.Counter(int(r[7]) for r in table if r[7] >= 0)
    prev_run = prev_lds = -1
    for r in table:
        width, run, tiny, lds = r[5] - r[0], int(r[7]), int(r[8]), int(r[9])
        if lds >= 0 and batch * 64 <= lds_limit:
            out[("b_lds", mode)] += lds != prev_lds
            prev_lds = lds
        elif run >= 0:
            if run != prev_run:
                out[("b_narrow_gate" if tiny == 1 else "b_narrow_class", mode)] += (run_len[run] + 1023) // 1024
            prev_run = run
        elif width:
            out[("b_full", mode)] += 1
    return {k: v for k, v in out.items() if v}


def add(*dicts):
    out = collections.Counter()
    for d in dicts:
        out.update(d)
    return dict(out)


def flip_in_record(proof: bytes, which: int) -> bytes:
    """the proof with one bit flipped inside the broadcast bytes (which even) or the correction bytes (odd) of a GF(2) record"""
    u64 = lambda at: struct.unpack_from("<Q", proof, at)[0]  # noqa: E731
    pos = 32
    n, pos = u64(pos), pos + 8
    spans = []
    for _ in range(n):
        pos += 1 + 128
        n_rec, pos = u64(pos), pos + 8
        rec, pos = pos, pos + n_rec
        n_corr, pos = u64(pos), pos + 8
        corr, pos = pos, pos + n_corr
        pos += 8 + u64(pos)
        spans.append(((rec, n_rec), (corr, n_corr)))
    at, length = spans[which % len(spans)][which & 1]
    if not length:
        at, length = spans[which % len(spans)][1 - (which & 1)]
    bad = bytearray(proof)
    bad[at + (which * 7919) % length] ^= 1 << (which % 8)
    return bytes(bad)


def answers(rv, oracle, c, prog, wc, proof: bytes):
    """(the library's, the oracle's) answer to a proof in compatibility mode and strict; None where the proof is refused"""
    def ask(f):
        try:
            return f()
        except (rv.ReverieError, oracle.OracleError):
            return None
    got = [ask(lambda s=s: rv.Proof(proof).verify(c, strict=s)) for s in (False, True)]
    want = [ask(lambda s=s: oracle.verify(prog, wc, proof, strict=s)) for s in (False, True)]
    return got, want


class Case:
    """one program: compiled once, its oracle proof computed once"""

    def __init__(self, rv, oracle, seeds, levels, rows_for, tag=0):
        self.rv, self.oracle, self.seeds, self.rows_for, self.tag = rv, oracle, seeds, set(rows_for), tag
        self.prog, self.wit, self.wc = cm.class_mix(levels, SEED)
        self.want = oracle.prove(self.prog, self.wit, [], self.wc, seeds)
        self.c = rv.Circuit(self.prog, self.wc, whole_prover=True)
        self.table, self.vclr_ok, self.general = circuit_levels(self.c)
        host = cm.level_table(self.prog, self.wc)
        # the circuit's plan is the host hook's: the same classes, the same runs
        assert [tuple(int(x) for x in (r[1] - r[0], r[2] - r[1], r[3] - r[2], r[4] - r[3], r[5] - r[4], r[6], r[7], r[8])) for r in self.table] == host
        assert [h[:5] for h in host] == cm.class_table(levels, SEED)
        self.seen = set()
        launches()

    def expect(self, want, what):
        got = launches()
        print(f"[{what}] launches {got}")
        assert got == want, what
        assert {k[0] for k in got} <= self.rows_for, what  # (none by an executor the case is not for)
        self.seen |= set(got)

    def whole(self, vc=True, tamper=True):
        """Proof.new, the strict verifier, one tampered proof"""
        rv, c = self.rv, self.c
        pmode = PV if self.vclr_ok else P
        vmode = VC if (vc and self.vclr_ok and not self.general) else V
        proof = rv.Proof.new(c, self.wit, [], seeds=self.seeds)
        self.expect(predict(self.table, 64, pmode), "prove")
        assert bytes(proof) == self.want
        from reverie_amd import _lib

        n_vc = _lib.lib().rv_hook_verify_vc_count()
        assert proof.verify(c, strict=True)
        self.expect(predict(self.table, 64, vmode), "verify")
        assert _lib.lib().rv_hook_verify_vc_count() - n_vc == (vmode == VC)
        if tamper:
            got, want = answers(rv, self.oracle, c, self.prog, self.wc, flip_in_record(self.want, self.tag))
            assert got == want
            launches()
        return pmode, vmode

    def shards(self, per):
        """the proof from repetition shards of `per` repetitions (the last one takes what is left)"""
        from reverie_amd.dist import HipShardBackend, assemble
        from reverie_amd.proof import challenge, combine_digests

        be = HipShardBackend(self.c)
        cuts = [(b, min(per, 256 - b)) for b in range(0, 256, per)]
        shards = [be.commit(self.wit, [], self.seeds[b:b + n], b, n) for b, n in cuts]
        try:
            comm = combine_digests(np.concatenate([be.digests(s) for s in shards]))
            omit = challenge(comm)
            parts = [be.open(s, omit)[:2] for s in shards]
        finally:
            for s in shards:
                be.destroy(s)
        self.expect(add(*[predict(self.table, n // 4, PV if self.vclr_ok and n // 4 in CLASS_NQ else P) for _, n in cuts]), f"shards of {per}")
        assert assemble(comm, parts) == self.want, per

    def groups(self, per):
        """the strict verifier over verifier groups, `per` groups of eight repetitions at a time"""
        from reverie_amd import _lib
        from reverie_amd.dist import HipShardBackend

        be = HipShardBackend(self.c)
        dig, zc, want = np.zeros((256, 32), np.uint8), True, []
        for g0 in range(0, 32, per):
            groups = list(range(g0, min(g0 + per, 32)))
            d, z = be.verify_groups(self.want, groups)
            for k, g in enumerate(groups):
                dig[8 * g:8 * g + 8] = d[8 * k:8 * k + 8]
            zc = zc and z
            want.append(predict(self.table, 2 * len(groups), V))
        self.expect(add(*want), f"verifier groups, {per} at a time")
        ok = C.c_int()
        buf = (C.c_uint8 * len(self.want)).from_buffer_copy(self.want)
        _lib.check(_lib.lib().rv_verify_finish_ex(buf, C.c_size_t(len(self.want)), dig.ctypes.data_as(C.c_void_p), C.c_uint32(0), C.c_int(int(zc)), C.byref(ok)))
        assert ok.value == 1, per

    def done(self):
        assert {k[0] for k in self.seen} == self.rows_for  # (every executor the case is for has run)


# ---------------------------------------------------------------- step remainders, launches of their own
@pytest.mark.parametrize("rand", [0, 1])
@pytest.mark.parametrize("cls", range(5))
@pytest.mark.parametrize("kind", ["fast", "alone", "general"])
def test_step_remainders_own_launches(rv, oracle, rule_seeds, monkeypatch, kind, cls, rand):
    """Two levels behind 300 Inputs, so every level is a launch of its own: class `cls` at 0, 1, S - 1, S, S + 1 and 2 S + 1 gates for
    the steps S = 4 (whole proofs, 64 quad words), 8 (shards of 128 and 64 repetitions) and 16 (shards of 32), and through the
    generic kernel (shards of 24) -- beside three gates of every other class, alone, or in a level of the general variant.  Without
    a Random op the prover runs MODE_PROVE_V and the verifier MODE_VERIFY_C (corr rows with RV_VERIFY_VC=0, and in a general
    level); with one, MODE_PROVE and MODE_VERIFY."""
    full = "full_general" if kind == "general" else "full_fast"
    for i, (name, levels) in enumerate(cm.step_specs(kind, cls, rand)):
        case = Case(rv, oracle, rule_seeds, levels, {"full_fast", full, "generic"}, tag=2 * i + cls)
        assert case.vclr_ok == (not rand) and case.general == (kind == "general"), name
        pmode, vmode = case.whole()
        assert (pmode, vmode) == ((P, V) if rand else (PV, V if kind == "general" else VC)), name
        assert (full, pmode) in case.seen and (full, vmode) in case.seen, name
        if not rand and kind != "general":
            monkeypatch.setenv("RV_VERIFY_VC", "0")
            assert case.whole(vc=False, tamper=False)[1] == V, name
            monkeypatch.delenv("RV_VERIFY_VC")
        for per in (128, 64, 32, 24):
            case.shards(per)
        for per in (16, 8, 4, 3):
            case.groups(per)
        case.done()


@pytest.mark.parametrize("i", range(len(cm.SLOT_SPECS)))
def test_slot_rotation_levels_of_a_few_gates(rv, oracle, rule_seeds, i):
    """a level of 1 to 5 gates in three classes: the class loops' first steps and the common loop share the first wavefronts"""
    name, levels = cm.SLOT_SPECS[i]
    case = Case(rv, oracle, rule_seeds, levels, {"full_fast", "generic"}, tag=i)
    case.whole()
    for per in (128, 64, 32, 24):
        case.shards(per)
    for per in (16, 8, 4, 3):
        case.groups(per)
    case.done()


# ---------------------------------------------------------------- the general switch
@pytest.mark.parametrize("c1,c3", cm.GENERAL_SWITCH)
def test_general_switch(rv, oracle, rule_seeds, monkeypatch, c1, c3):
    """c1 + c3 at 63, 64 and 65 in a level of 300 gates (a launch of its own: the variant changes at 64, and MODE_VERIFY_C is not
    taken with a general level) and inside a class-loop narrow run (never lean)"""
    general = c1 + c3 >= 64
    full = "full_general" if general else "full_fast"
    for rand in (0, 1):
        case = Case(rv, oracle, rule_seeds, cm.switch_own(c1, c3, rand), {"full_fast", full}, tag=c1 + rand)
        assert case.general == general
        pmode, vmode = case.whole()
        assert (pmode, vmode) == ((P, V) if rand else (PV, V if general else VC))
        assert case.seen >= {(full, pmode), (full, vmode)}
        for per in (128, 32):
            case.shards(per)
        case.done()
    for lds in ("0", None):
        if lds:
            monkeypatch.setenv("RV_LDS_RUN", lds)
        else:
            monkeypatch.delenv("RV_LDS_RUN")
        case = Case(rv, oracle, rule_seeds, cm.switch_in_run(c1, c3), {"full_fast", "lds"} if lds is None else {"full_fast", "narrow_class", "narrow_gate"}, tag=c3)
        assert (case.table[:, 9] >= 0).any() == (lds is None)
        assert case.whole() == (P, V)
        if lds:
            assert case.seen >= {("narrow_class", P), ("narrow_class", V), ("narrow_gate", P), ("narrow_gate", V)}
        case.done()


# ---------------------------------------------------------------- MODE_PROVE_V's limit
def test_vclr_limit_16_narrow_levels(rv, oracle, rule_seeds, monkeypatch):
    """16 levels in narrow runs: every level launched on its own by MODE_PROVE_V and MODE_VERIFY_C; a 17th moves the whole circuit
    to the run executors"""
    monkeypatch.setenv("RV_LDS_RUN", "0")
    case = Case(rv, oracle, rule_seeds, cm.VCLR_SPECS[16], {"full_fast"})
    assert case.vclr_ok and case.whole() == (PV, VC)
    assert case.seen == {("full_fast", PV), ("full_fast", VC)}
    case.done()
    case = Case(rv, oracle, rule_seeds, cm.VCLR_SPECS[17], {"full_fast", "narrow_gate"})
    assert not case.vclr_ok and case.whole() == (P, V)
    assert case.seen == {("full_fast", P), ("full_fast", V), ("narrow_gate", P), ("narrow_gate", V)}
    case.done()
    monkeypatch.delenv("RV_LDS_RUN")
    case = Case(rv, oracle, rule_seeds, cm.VCLR_SPECS[17], {"full_fast", "lds"})
    assert not case.vclr_ok and case.whole() == (P, V)
    case.done()


# ---------------------------------------------------------------- run planning
RUN_KERNELS = {"two-then-three": {"narrow_gate"}, "7x33-8x33-8x32": {"narrow_gate", "narrow_class"}, "256": {"narrow_gate"}, "257": set(),
               "merge": {"narrow_gate"}, "lean": {"narrow_lean", "narrow_gate"}, "not-lean": {"narrow_class", "narrow_gate"},
               "window": {"narrow_class"}, "1025": {"narrow_class"}}


@pytest.mark.parametrize("lds", ["0", None])
@pytest.mark.parametrize("name", sorted(cm.RUN_SPECS))
def test_run_plans(rv, oracle, rule_seeds, monkeypatch, name, lds):
    """The narrow-run plan at its split points, with the row interpreter's narrow kernels (RV_LDS_RUN=0) and with LDS runs wherever
    the circuit's plan reports one; whole proofs, and shards of 128 and 24 repetitions (class loops of 8 gates, and the per-gate
    kernel in place of a class-loop one)"""
    if lds:
        monkeypatch.setenv("RV_LDS_RUN", lds)
    levels, runs = cm.RUN_SPECS[name]
    case = Case(rv, oracle, rule_seeds, levels, set(ROWS[:7]), tag=len(name))
    in_run, in_lds = case.table[:, 7] >= 0, case.table[:, 9] >= 0
    print(f"[{name}] LDS runs over {int(in_lds.sum())} of {int(in_run.sum())} run levels")
    assert not in_lds[~in_run].any() and not (lds and in_lds.any())
    assert case.whole() == (P, V)
    rows = {k[0] for k in case.seen}
    if lds:
        assert rows == {"full_fast"} | RUN_KERNELS[name] and {k[1] for k in case.seen} == {P, V}, name
    elif in_lds[in_run].all():
        assert rows == ({"full_fast", "lds"} if runs else {"full_fast"}), name
    if name == "1025" and lds:
        assert predict(case.table, 64, P)[("narrow_class", P)] == 2  # 1 025 levels: two launches
    for per in (128, 24):
        case.shards(per)
    case.groups(16)
    case.groups(3)


# ---------------------------------------------------------------- batches
@pytest.mark.parametrize("limit", [None, "0", "100000"])
def test_batches(rv, oracle, rule_seeds, monkeypatch, limit):
    """Proof.new_batch of three witnesses and verify_batch: a circuit of own launches with all five classes at remainders of 4
    (k_interp_full_b: always the general variant), and narrow runs with multi-base gates (k_interp_narrow_b has no lean variant)
    through LDS runs and, with RV_LDS_BATCH_WGS=0, through the batched narrow kernels"""
    if limit is not None:
        monkeypatch.setenv("RV_LDS_BATCH_WGS", limit)
    lim = 768 if limit is None else int(limit)
    nb = 3
    seeds = np.stack([np.roll(rule_seeds, b, axis=0) for b in range(nb)])
    for levels, rows in ((cm.BATCH_OWN, {"b_full"}), (cm.BATCH_RUN, {"b_full", "b_lds"} if lim else {"b_full", "b_narrow_gate", "b_narrow_class"})):
        case = Case(rv, oracle, rule_seeds, levels, rows)
        wants = [case.want] + [oracle.prove(case.prog, case.wit, [], case.wc, seeds[b]) for b in range(1, nb)]
        got = rv.Proof.new_batch(case.c, np.tile(np.asarray(case.wit, np.uint8), (nb, 1)), seeds=seeds)
        case.expect(predict_batch(case.table, nb, P, lim), "new_batch")
        assert [bytes(g) for g in got] == wants
        assert rv.verify_batch(case.c, got, strict=True) == [True] * nb
        case.expect(predict_batch(case.table, nb, V, lim), "verify_batch")
        bad = [wants[0], flip_in_record(wants[1], 4), wants[2]]
        want_bad = answers(rv, oracle, case.c, case.prog, case.wc, bad[1])[1][1]
        launches()
        assert rv.verify_batch(case.c, bad, strict=True) == [True, bool(want_bad), True]
        launches()
        case.done()


# ---------------------------------------------------------------- the grid cap and the prefetch plan
@pytest.mark.parametrize("name", sorted(cm.GRID_SPECS))
def test_grid_cap_and_prefetch(rv, oracle, rule_seeds, name):
    """A level of 70 000 gates: more than 4 096 workgroups take in one pass, so the grid-stride loops of k_interp_full go round
    twice (both variants).  A level of 20 000 gates in front of a level of one gate, and a last level with class loops: the
    prefetch plan with a tiny next level and with none."""
    general = name == "cap-general"
    case = Case(rv, oracle, rule_seeds, cm.GRID_SPECS[name], {"full_fast", "full_general"} if general else {"full_fast"}, tag=3)
    assert case.general == general
    assert case.whole() == (PV, V if general else VC)
    case.done()


# ---------------------------------------------------------------- every executor, every mode that reaches it
def test_every_executor_runs_in_every_mode_that_reaches_it(rv, oracle, rule_seeds, monkeypatch):
    """The table of rv_hook_interp_launches over a handful of the cases above: each executor non-zero in every mode it has --
    the launches of their own in all four (the generic kernel exists as PROVE and VERIFY only: launch_interp), the narrow, LDS and
    batched executors as PROVE and VERIFY (MODE_PROVE_V and MODE_VERIFY_C launch every level on its own: shard_run_levels)"""
    seen = set()
    for rand in (0, 1):
        for kind in ("fast", "general"):
            case = Case(rv, oracle, rule_seeds, [cm.wide0(rand), cm.step_mix(kind, 0, 5)], set(ROWS))
            case.whole(tamper=False)
            if kind == "fast" and not rand:
                monkeypatch.setenv("RV_VERIFY_VC", "0")
                case.whole(vc=False, tamper=False)
                monkeypatch.delenv("RV_VERIFY_VC")
            case.shards(24)
            case.groups(3)
            seen |= case.seen
    # (a general level under MODE_VERIFY_C does not exist: verify.inc takes MODE_VERIFY for a circuit with one)
    for lds in ("0", None):
        if lds:
            monkeypatch.setenv("RV_LDS_RUN", lds)
        else:
            monkeypatch.delenv("RV_LDS_RUN")
        for name in ("lean", "not-lean"):
            case = Case(rv, oracle, rule_seeds, cm.RUN_SPECS[name][0], set(ROWS))
            case.whole(tamper=False)
            seen |= case.seen
    seeds = np.stack([rule_seeds, rule_seeds[::-1]])
    for limit in ("0", "100000"):
        monkeypatch.setenv("RV_LDS_BATCH_WGS", limit)
        case = Case(rv, oracle, rule_seeds, cm.BATCH_RUN, set(ROWS))
        got = rv.Proof.new_batch(case.c, np.tile(np.asarray(case.wit, np.uint8), (2, 1)), seeds=seeds)
        case.expect(predict_batch(case.table, 2, P, int(limit)), "new_batch")
        assert bytes(got[0]) == case.want
        assert rv.verify_batch(case.c, got, strict=True) == [True, True]
        case.expect(predict_batch(case.table, 2, V, int(limit)), "verify_batch")
        seen |= case.seen
    want = {("full_fast", m) for m in (P, PV, V, VC)} | {("full_general", m) for m in (P, PV, V)}
    want |= {(r, m) for r in ROWS[2:] for m in (P, V)}
    assert seen == want, sorted(want ^ seen)
