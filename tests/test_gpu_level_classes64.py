"""Every Z64 level executor against the oracle, level by gate-class mix and by value.  tests/class_mix64.py builds Z64 programs whose
compiled levels hold a chosen number of Mul, linear and other gates (test_class_mix64_host.py pins on the host that each spec compiles
to its counts and hits the split of k_z64_fused's launch grid and wavefront deal it is named for); here every one of them is proved and
verified on the GPU on every executor that takes it -- the proof byte for byte the oracle's, the strict verifier accepting it -- and
rv_hook_interp64_launches must show, around every call, one launch per Z64 level by the executor the call is for and none by any other:

    k_z64_fused<16>, prove     Proof.new; repetition shards of 128 and 64 (two and one quad group: other chunk counts)
    k_z64_fused<8>, prove      shards of 32
    k_z64_fused<16>, verify    Proof.verify (RV_Z64_FUSED_VERIFY unset), two passes over the levels when the schedule is split64; verifier
                               groups, eight at a time (one quad group)
    k_z64_fused<8>, verify     verifier groups, four at a time
    k_interp64, prove          RV_Z64_FUSED=0; the specs that are not eligible; shards of 24 (96 lanes per gate in workgroups of 256)
    k_interp64, verify         RV_Z64_FUSED_VERIFY=0; the specs that are not eligible; verifier groups, three at a time
    k_interp64_b, both         Proof.new_batch / verify_batch of two and three proofs

For a handful of specs the verifiers also answer one bit flip in every Z64 section of the proof (tests/proof_mutate.py) and a program
whose last SubConst immediate is off by one as the oracle does, strict and not, on both verifier executors."""
import ctypes as C

import numpy as np
import pytest

import class_mix64 as cm
import proof_mutate
from test_gpu_verify_groups import span_bytes

pytestmark = pytest.mark.gpu

ROWS = ["fused16", "fused8", "interp64", "interp64_b"]
P, V = 0, 1
SIDE_COPY_BYTES = 4 << 20  # (csrc/verify.inc: verify_schedule)
NAMES = sorted(cm.all_specs(256))  # (the names do not depend on the compute units; the sizes of some specs do)
BATCH_BELOW = 1000  # ops: the specs that also run as a batch of two proofs
TAMPERED = ["mixed", "mixed-edges", "rotation-edges", "interleaved", "odd-inputs", "deal4-plenty-3", "only-az"]


@pytest.fixture(scope="module")
def rv():
    """the package, with a context of this file's own: its arena (a hundred circuits of as many sizes, every executor's scratch) goes
    back to the device when the file is done, and the context the other files share keeps the memory it had"""
    import reverie_amd

    Case.ctx = reverie_amd.Context(0)
    yield reverie_amd
    Case.ctx.close()
    Case.ctx = None


@pytest.fixture(scope="module")
def specs(rv):
    return cm.all_specs(cm.machine_cus())


@pytest.fixture(autouse=True)
def _plain_env(monkeypatch):
    for k in ("RV_Z64_FUSED", "RV_Z64_FUSED_VERIFY"):
        monkeypatch.delenv(k, raising=False)


def launches():
    """the launches since the last call -> {(executor, column): count}"""
    from reverie_amd import _lib

    counts = ((C.c_uint64 * 2) * len(ROWS))()
    _lib.check(_lib.lib().rv_hook_interp64_launches(counts, C.c_int(1)))
    return {(ROWS[e], m): int(counts[e][m]) for e in range(len(ROWS)) for m in range(2) if counts[e][m]}


def schedule():
    from reverie_amd import _lib

    out = (C.c_uint64 * 8)()
    _lib.check(_lib.lib().rv_hook_verify_schedule(out))
    return [int(x) for x in out]


def answer(f, errors):
    """(value, None), or (None, the error code)"""
    try:
        return f(), None
    except errors as e:
        return None, e.code


class Case:
    """one spec: built once, its oracle proof computed once, one circuit for every executor"""
    ctx = None

    def __init__(self, rv, oracle, seeds, spec):
        self.rv, self.oracle, self.seeds, self.spec = rv, oracle, seeds, spec
        self.prog, self.wit, self.wc, self.table = cm.build(spec)
        self.n = len(self.table)  # (every level holds gates: one launch each)
        self.want = oracle.prove(self.prog, [], self.wit, self.wc, seeds)
        self.c = rv.Circuit(self.prog, self.wc, Case.ctx)
        self.fused = spec.why == cm.ELIGIBLE
        got, why = cm.fused_levels(self.prog, self.wc)
        assert got == self.table and why == spec.why  # (what test_class_mix64_host.py pins, on this machine's compute units)
        self.seen = set()
        launches()

    def expect(self, want, what):
        got = launches()
        print(f"[{self.spec.name}: {what}] {got}")
        assert got == want, (self.spec.name, what)
        self.seen |= set(got)

    def prove(self, monkeypatch, fused=True):
        if not fused:
            monkeypatch.setenv("RV_Z64_FUSED", "0")
        proof = self.rv.Proof.new(self.c, [], self.wit, seeds=self.seeds)
        monkeypatch.delenv("RV_Z64_FUSED", raising=False)
        self.expect({("fused16" if fused and self.fused else "interp64", P): self.n}, f"prove fused={fused}")
        assert bytes(proof) == self.want, (self.spec.name, fused)

    def verify(self, monkeypatch, fused=True, split=False):
        if not fused:
            monkeypatch.setenv("RV_Z64_FUSED_VERIFY", "0")
        s0 = schedule()
        ok = self.rv.Proof(self.want).verify(self.c, strict=True)
        monkeypatch.delenv("RV_Z64_FUSED_VERIFY", raising=False)
        delta = [a - b for a, b in zip(schedule(), s0)]
        on = fused and self.fused
        assert (delta[0], delta[3], delta[4]) == (1, int(split and on), int(on)), (self.spec.name, delta)
        self.expect({("fused16" if on else "interp64", V): self.n * (2 if split and on else 1)}, f"verify fused={fused}")
        assert ok is True, (self.spec.name, fused)

    def shards(self, per):
        """the proof from repetition shards of `per` repetitions (the last one takes what is left)"""
        from reverie_amd.dist import HipShardBackend, assemble
        from reverie_amd.proof import challenge, combine_digests

        be = HipShardBackend(self.c)
        cuts = [(b, min(per, 256 - b)) for b in range(0, 256, per)]
        shards = [be.commit([], self.wit, self.seeds[b:b + n], b, n) for b, n in cuts]
        try:
            comm = combine_digests(np.concatenate([be.digests(s) for s in shards]))
            omit = challenge(comm)
            parts = [be.open(s, omit)[:2] for s in shards]
        finally:
            for s in shards:
                be.destroy(s)
        want = {}
        for _, n in cuts:
            nq = n // 4
            row = "interp64" if not self.fused or nq % 8 else "fused16" if nq % 16 == 0 else "fused8"
            want[(row, P)] = want.get((row, P), 0) + self.n
        self.expect(want, f"shards of {per}")
        assert assemble(comm, parts) == self.want, (self.spec.name, per)

    def groups(self, per):
        """the strict verifier over verifier groups, `per` groups of eight repetitions at a time: rows of 2 * per quad words"""
        from reverie_amd import _lib
        from reverie_amd.dist import HipShardBackend

        be = HipShardBackend(self.c)
        dig, zc, want = np.zeros((256, 32), np.uint8), True, {}
        for g0 in range(0, 32, per):
            groups = list(range(g0, min(g0 + per, 32)))
            d, z = be.verify_groups(self.want, groups)
            for k, g in enumerate(groups):
                dig[8 * g:8 * g + 8] = d[8 * k:8 * k + 8]
            zc = zc and z
            nq = 2 * len(groups)
            row = "interp64" if not self.fused or nq % 8 else "fused16" if nq % 16 == 0 else "fused8"
            want[(row, V)] = want.get((row, V), 0) + self.n
        self.expect(want, f"verifier groups, {per} at a time")
        ok = C.c_int()
        buf = (C.c_uint8 * len(self.want)).from_buffer_copy(self.want)
        _lib.check(_lib.lib().rv_verify_finish_ex(buf, C.c_size_t(len(self.want)), dig.ctypes.data_as(C.c_void_p), C.c_uint32(0), C.c_int(int(zc)), C.byref(ok)))
        assert ok.value == 1, (self.spec.name, per)

    def batch(self, nb):
        rv = self.rv
        seeds = np.stack([np.roll(self.seeds, b, axis=0) for b in range(nb)])
        wants = [self.want] + [self.oracle.prove(self.prog, [], self.wit, self.wc, seeds[b]) for b in range(1, nb)]
        got = rv.Proof.new_batch(self.c, np.zeros((nb, 0), np.uint8), np.tile(np.asarray(self.wit, np.uint64), (nb, 1)), seeds=seeds)
        self.expect({("interp64_b", P): self.n}, f"new_batch of {nb}")
        assert [bytes(g) for g in got] == wants, self.spec.name
        assert rv.verify_batch(self.c, got, strict=True) == [True] * nb
        self.expect({("interp64_b", V): self.n}, f"verify_batch of {nb}")
        bad = list(wants)
        bad[nb - 1] = flip(wants[nb - 1], "corr", 2)
        want_bad = answer(lambda: self.oracle.verify(self.prog, self.wc, bad[nb - 1], strict=True), self.oracle.OracleError)
        if want_bad[1] is None:
            assert rv.verify_batch(self.c, bad, strict=True) == [True] * (nb - 1) + [want_bad[0]]
        launches()

    def everything(self, monkeypatch):
        self.prove(monkeypatch)
        self.verify(monkeypatch)
        self.prove(monkeypatch, fused=False)
        self.verify(monkeypatch, fused=False)
        for per in (128, 64, 32, 24):
            self.shards(per)
        for per in (8, 4, 3):
            self.groups(per)
        if len(self.prog) < BATCH_BELOW:
            self.batch(2)
        rows = {("interp64", P), ("interp64", V)}
        if self.fused:
            rows |= {("fused16", P), ("fused16", V), ("fused8", P), ("fused8", V)}
        if len(self.prog) < BATCH_BELOW:
            rows |= {("interp64_b", P), ("interp64_b", V)}
        assert self.seen == rows, (self.spec.name, sorted(self.seen ^ rows))


def flip(proof: bytes, section: str, which: int) -> bytes:
    """the proof with one bit flipped in a Z64 section: the keys, rec, corr or in bytes of an online record, or the preprocessing
    pairs (seed | commitment) of the unopened repetitions (an empty section: the record's keys)"""
    comm, doms = proof_mutate.parse(proof)
    doms = proof_mutate._copy(doms)
    records, pre = doms[1]
    if section == "pre":
        b = bytearray(pre)
        b[(which * 7919) % len(b)] ^= 1 << (which % 8)
        doms[1] = (records, bytes(b))
    else:
        rec = records[which % len(records)]
        if section != "keys" and not rec[2][proof_mutate.VECTORS.index(section)]:
            section = "keys"  # (a program without the gates that fill the section: the record's keys instead)
        b = bytearray(rec[1] if section == "keys" else rec[2][proof_mutate.VECTORS.index(section)])
        b[(which * 7919) % len(b)] ^= 1 << (which % 8)
        if section == "keys":
            rec[1] = bytes(b)
        else:
            rec[2][proof_mutate.VECTORS.index(section)] = bytes(b)
    out = proof_mutate.serialise(comm, doms)
    assert len(out) == len(proof) and out != proof
    return out


# ---------------------------------------------------------------- every spec on every executor that takes it
@pytest.mark.parametrize("name", [n for n in NAMES if n != "split64"])
def test_spec_on_every_executor(rv, oracle, rule_seeds, monkeypatch, specs, name):
    """Proof.new and the strict verifier fused and through k_interp64, shards of 128 / 64 / 32 / 24 repetitions, and -- the smaller
    specs -- a batch of two proofs; a spec that is not eligible runs k_interp64 wherever the fused kernel would have run"""
    spec = specs[name]
    case = Case(rv, oracle, rule_seeds, spec)
    if spec.at is not None and case.fused and (name.startswith("sat-") or name.startswith("chunk-")):
        # (sized by this machine's compute units: the branch and the deal are what the name says here too)
        cus = cm.machine_cus()
        br, deal, _ = cm.level_labels(case.table[spec.at], 16, 4, cus)
        print(f"[{name}] cus {cus}: {sorted(br)} {sorted(deal)}")
        if name.startswith("sat-"):
            reg, x = name.split("-")[1:]
            assert {d[:2] for d in deal} == {(reg, int(x))} and br & {"saturated", "at-per_qg"} and not any(d[2] for d in deal)
        else:
            assert cm.chunk_specs(cus)[name[len("chunk-"):]][2] in br
    case.everything(monkeypatch)


def test_ineligible_specs_run_the_two_kernel_path(rv, oracle, rule_seeds, monkeypatch, specs):
    """an odd number of Inputs in front of the first Mul, and 65 Input block runs: never a fused launch; 64 runs: fused"""
    for name, fused in (("odd-inputs", False), ("runs-65", False), ("runs-64", True)):
        case = Case(rv, oracle, rule_seeds, specs[name])
        assert case.fused == fused
        case.prove(monkeypatch)
        case.verify(monkeypatch)
        assert {k[0] for k in case.seen} == ({"fused16"} if fused else {"interp64"}), name


# ---------------------------------------------------------------- past the caps of the two-kernel path
def test_k_interp64_past_its_grid_cap(rv, oracle, rule_seeds, monkeypatch, specs):
    """a level of 2 100 linear gates: more than the 2 048 workers of 8 192 workgroups at 256 repetitions, the grid-stride loop goes
    round twice -- prover and verifier (and the fused kernel on the same level: chunks by row traffic alone)"""
    case = Case(rv, oracle, rule_seeds, specs["wide-lin"])
    assert sum(case.table[1]) > 8192 * 256 // (256 * 4) and case.table[1][0] == 0
    case.prove(monkeypatch, fused=False)
    case.verify(monkeypatch, fused=False)
    assert case.seen == {("interp64", P), ("interp64", V)}


@pytest.mark.parametrize("name,nb", [("batch-small", 2), ("batch-small", 3), ("batch-wide", 3), ("mixed-edges", 3)])
def test_batches(rv, oracle, rule_seeds, specs, name, nb):
    """Proof.new_batch and verify_batch (k_interp64_b, both modes); batch-wide: a level of 703 gates against the 8192 / 4 / 3 = 682
    workers a proof gets in a batch of three"""
    case = Case(rv, oracle, rule_seeds, specs[name])
    if name == "batch-wide":
        assert sum(case.table[1]) > 8192 // 4 // nb
    case.batch(nb)
    assert case.seen == {("interp64_b", P), ("interp64_b", V)}


# ---------------------------------------------------------------- split64
def test_fused_verifier_split64_smallest_proof(rv, oracle, rule_seeds, monkeypatch, specs):
    """The smallest proof of its shape whose online records reach the 4 MiB from which the verifier copies them on the side stream:
    the fused verifier then runs the quad groups without an opened repetition first and the first quad group behind the copy --
    two passes over the levels, both counted.  One Mul gate less (with its sink gates: 960 bytes of records) stays below."""
    case = Case(rv, oracle, rule_seeds, specs["split64"])
    span = span_bytes(case.want, range(5))
    assert SIDE_COPY_BYTES <= span < SIDE_COPY_BYTES + 960, span
    case.prove(monkeypatch)
    case.verify(monkeypatch, split=True)
    case.verify(monkeypatch, fused=False)
    assert case.seen == {("fused16", P), ("fused16", V), ("interp64", V)}
    bad = flip(case.want, "corr", 5)
    for strict in (False, True):
        want = answer(lambda: oracle.verify(case.prog, case.wc, bad, strict=strict), oracle.OracleError)
        assert answer(lambda: rv.Proof(bad).verify(case.c, strict=strict), rv.ReverieError) == want


# ---------------------------------------------------------------- the verifiers on altered proofs
@pytest.mark.parametrize("fused_verify", ["1", "0"])
@pytest.mark.parametrize("name", TAMPERED)
def test_verifiers_answer_altered_proofs_as_the_oracle(rv, oracle, rule_seeds, monkeypatch, specs, name, fused_verify):
    """the valid proof strict and not; one bit flip in each Z64 section; a program whose last SubConst immediate is off by one"""
    case = Case(rv, oracle, rule_seeds, specs[name])
    monkeypatch.setenv("RV_Z64_FUSED_VERIFY", fused_verify)
    errors = (rv.ReverieError, oracle.OracleError)
    for strict in (False, True):
        assert rv.Proof(case.want).verify(case.c, strict=strict) is True
    row = "fused16" if case.fused and fused_verify == "1" else "interp64"
    case.expect({(row, V): 2 * case.n}, "valid proof, twice")
    tag = sum(map(ord, name))
    for k, section in enumerate(("keys", "rec", "corr", "in", "pre")):
        bad = flip(case.want, section, tag + k)
        for strict in (False, True):
            want = answer(lambda: oracle.verify(case.prog, case.wc, bad, strict=strict), errors)
            got = answer(lambda: rv.Proof(bad).verify(case.c, strict=strict), errors)
            assert got == want, (name, section, strict)
        assert set(launches()) <= {(row, V)}, (name, section)
    idx = np.flatnonzero((case.prog["domain"] == 1) & (case.prog["opcode"] == 5))
    assert len(idx)
    bad_prog = case.prog.copy()
    bad_prog[idx[-1]]["imm"] ^= 1
    bad_c = rv.Circuit(bad_prog, case.wc, Case.ctx)
    for strict in (False, True):
        want = answer(lambda: oracle.verify(bad_prog, case.wc, case.want, strict=strict), errors)
        got = answer(lambda: rv.Proof(case.want).verify(bad_c, strict=strict), errors)
        assert got == want, (name, "SubConst off by one", strict)


# ---------------------------------------------------------------- the whole table
def test_every_z64_executor_runs_in_both_modes(rv, oracle, rule_seeds, monkeypatch, specs):
    """the table of rv_hook_interp64_launches over one small spec: every executor non-zero in both modes"""
    case = Case(rv, oracle, rule_seeds, specs["batch-small"])
    case.everything(monkeypatch)
    assert case.seen == {(r, m) for r in ROWS for m in (P, V)}
