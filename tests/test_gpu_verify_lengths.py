"""Every verifier entry point on WELL-FORMED proofs whose vector lengths were altered (tests/proof_mutate.py): the oracle's
answer -- accepted, refused or malformed, strict and reference-compatible -- is the only right one.

The reference takes a vector's length from the group's first record, reads zero past a vector's end and ignores bytes past
what the circuit consumes (oracle/rv_oracle.c verify_group); the library restates that in check_records / fill_slots, in the
masked word staging of k_unpack_bits, in k_unpack64, in the compact-corrections and fused Z64 verifiers, in rv_verify_batch
and in the streaming verifiers, where a chunk's supplied values start at any bit of a vector.  Honest vectors have one
length only, so nothing else reaches these rules.

Circuits, catalogues and the oracle's answers (computed once per process): tests/verify_length_cases.py.

The cases of one circuit share its catalogue; an entry point that takes long is split into several cases (the streaming
verifier by its cuts, the group split by its world).

THINNED AXIS: the streaming verifiers and the group split run the catalogue's THIN target axis (record 0, record 3 and all
eight records of groups 0 and 4; record 7 and all-40 are left to the other entry points) -- they start several device passes
per entry.  The length changes are never thinned."""
import pytest

import proof_mutate
import verify_length_cases as cases
from test_gpu_verify_groups import COMPAT, finish, lists, verify_split

pytestmark = pytest.mark.gpu

MALFORMED = ("err", 4)  # RV_E_PROOF_MALFORMED == RVO_E_PROOF_MALFORMED
MODES = ((True, 0), (False, 1))  # (strict, index into an oracle answer)
ENV = {  # the environment variants rv_verify_ex runs under (None: unset)
    "MIX": [{}],
    "WIDE": [{"RV_VERIFY_VC": None}, {"RV_VERIFY_VC": "0"}],
    "Z": [{"RV_Z64_FUSED_VERIFY": None}, {"RV_Z64_FUSED_VERIFY": "0"}],
}
BATCH = 24  # altered proofs per batched call (with their good neighbours: 49 proofs)


@pytest.fixture(scope="module")
def rv():
    import reverie_amd

    reverie_amd.Context.default()
    return reverie_amd


_cases = {}


@pytest.fixture
def case(rv, oracle, rule_seeds, name):
    """the circuit's catalogue with the oracle's answers, Proof objects (read in place by every call) and the compiled circuit"""
    if name not in _cases:
        cs = dict(cases.case(oracle, rule_seeds, name))
        assert bytes(rv.Proof.new(cs["prog"], cs["w2"], cs["w64"], cs["wc"], seeds=rule_seeds)) == cs["good"]
        cs["good_p"] = rv.Proof(cs["good"])
        cs["proofs"] = [rv.Proof(data) for _, data in cs["entries"]]
        cs["circuit"] = rv.Circuit(cs["prog"], cs["wc"])
        thin = {e[0] for e in proof_mutate.catalogue(cs["good"], targets=proof_mutate.THIN_TARGETS, gf2_items=cases.gf2_items(cs["prog"]))}
        cs["thin"] = [i for i, e in enumerate(cs["entries"]) if e[0] in thin]
        cs["label_at"] = {e[0]: i for i, e in enumerate(cs["entries"])}
        n_true, n_false, n_bad = cases.classes(cs["answers"])
        assert min(n_true, n_false, n_bad) >= 10, (n_true, n_false, n_bad)
        _cases[name] = cs
    return _cases[name]


def got(fn, *args, **kw):
    """what a verifier call answers: a bool, or ("err", code)"""
    from reverie_amd import ReverieError

    try:
        return bool(fn(*args, **kw))
    except ReverieError as e:
        return ("err", e.code)


class Report:
    """collects every disagreement, so that one run names all the labels"""

    def __init__(self, what):
        self.what, self.bad, self.n = what, [], 0

    def check(self, label, variant, have, want):
        self.n += 1
        if have != want:
            self.bad.append(f"{label} [{variant}]: {have!r}, the oracle says {want!r}")

    def done(self):
        assert not self.bad, f"{self.what}: {len(self.bad)} of {self.n} answers differ from the oracle's:\n  " + "\n  ".join(self.bad[:40])
        assert self.n > 0


def set_env(monkeypatch, env):
    for k, v in env.items():
        if v is None:
            monkeypatch.delenv(k, raising=False)
        else:
            monkeypatch.setenv(k, v)


def fused_eligible(rv, prog, wc, monkeypatch):
    """whether the circuit takes the fused Z64 kernels (the verifier's too, unless RV_Z64_FUSED_VERIFY=0).  There is no counter
    for that path; a circuit that takes it keeps a second, sorted copy of its Z64 gates on the device, which its device bytes
    show against a compile with RV_Z64_FUSED=0.  (Rows of 64 quad words -- a whole proof -- are a width the kernels support.)"""
    monkeypatch.setenv("RV_Z64_FUSED", "0")
    plain = rv.Circuit(prog, wc)
    monkeypatch.delenv("RV_Z64_FUSED")
    fused = rv.Circuit(prog, wc)
    try:
        return fused.info["device_bytes"] > plain.info["device_bytes"]
    finally:
        plain.close()
        fused.close()


# ---- 1. rv_verify_ex on the compiled circuit
def run_verify_ex(rv, name, cs, monkeypatch):
    from reverie_amd import _lib

    hook = _lib.lib().rv_hook_verify_vc_count
    rep = Report(f"{name} rv_verify_ex")
    if name == "Z":
        assert fused_eligible(rv, cs["prog"], cs["wc"], monkeypatch)
    for env in ENV[name]:
        set_env(monkeypatch, env)
        n0 = hook()
        assert cs["good_p"].verify(cs["circuit"]) and cs["good_p"].verify(cs["circuit"], strict=False)
        if name == "WIDE":  # the compact-corrections verifier is what runs, unless it is switched off
            assert hook() - n0 == (0 if env["RV_VERIFY_VC"] == "0" else 2), env
        for (label, _), p, want in zip(cs["entries"], cs["proofs"], cs["answers"]):
            for strict, k in MODES:
                rep.check(label, f"strict={strict} {env}", got(p.verify, cs["circuit"], strict=strict), want[k])
        if name == "WIDE":
            assert (hook() - n0 == 0) if env["RV_VERIFY_VC"] == "0" else (hook() - n0 > 2), env
    rep.done()


# ---- 2. rv_verify_ops: the raw op list
def run_verify_ops(rv, name, cs, monkeypatch):
    rep = Report(f"{name} rv_verify_ops")
    for (label, _), p, want in zip(cs["entries"], cs["proofs"], cs["answers"]):
        for strict, k in MODES:
            rep.check(label, f"strict={strict}", got(p.verify, cs["prog"], cs["wc"], strict=strict), want[k])
    rep.done()


# ---- 3. / 5. the batched verifiers: [good, e1, good, e2, ..., good]; a malformed proof is False, its neighbours are not touched
def check_batched(rep, cs, idx, verify, variant):
    for at in range(0, len(idx), BATCH):
        part = idx[at:at + BATCH]
        proofs = [cs["good_p"]]
        for i in part:
            proofs += [cs["proofs"][i], cs["good_p"]]
        for strict, k in MODES:
            oks = verify(proofs, strict)
            assert len(oks) == len(proofs)
            for j, ok in enumerate(oks[0::2]):
                near = [cs["entries"][i][0] for i in part[max(j - 1, 0):j + 1]]
                rep.check(f"good neighbour of {near}", f"strict={strict} {variant}", ok, True)
            for i, ok in zip(part, oks[1::2]):
                want = cs["answers"][i][k]
                rep.check(cs["entries"][i][0], f"strict={strict} {variant}", ok, False if want == MALFORMED else want)


def run_verify_batch(rv, name, cs, monkeypatch):
    rep = Report(f"{name} rv_verify_batch")
    every = list(range(len(cs["entries"])))
    for batch_max in (None, "4"):
        set_env(monkeypatch, {"RV_BATCH_MAX": batch_max})
        check_batched(rep, cs, every, lambda proofs, strict: rv.verify_batch(cs["circuit"], proofs, strict=strict), f"RV_BATCH_MAX={batch_max}")
    rep.done()


def run_stream_batch(rv, name, cs, monkeypatch, chunk_ops):
    from reverie_amd.stream import verify_streaming_batch

    rep = Report(f"{name} rv_verify_streaming_batch")
    check_batched(rep, cs, cs["thin"], lambda proofs, strict: verify_streaming_batch(cs["prog"], cs["wc"], proofs, strict=strict, max_chunk_ops=chunk_ops),
                  f"max_chunk_ops={chunk_ops}")
    rep.done()


# ---- 4. the streaming verifier
def stream_verify(proof, prog, wc, cuts, strict, device_compile=False):
    from reverie_amd.stream import StreamingVerifier

    sv = StreamingVerifier(wc, proof, device_compile=device_compile)
    try:
        edges = [0] + sorted(set(int(c) for c in cuts if 0 < c < len(prog))) + [len(prog)]
        for a, b in zip(edges[:-1], edges[1:]):
            sv.feed(prog[a:b])
        return sv.finish(strict=strict)
    finally:
        sv.close()


def boundary_cuts(cs, label):
    """for an entry that SHORTENS `in` or `corr`: cut sets that put a piece boundary before, exactly at and after the op that
    consumes the first item past the vector's new end, and one that leaves two whole later pieces past it"""
    dom, vec, group, target, change = proof_mutate.split_label(label)
    if vec not in ("in", "corr") or dom not in proof_mutate.DOMAINS or change.startswith("+") or change == "padbits":
        return []
    d = proof_mutate.DOMAINS.index(dom)
    first = proof_mutate.target_records((target, group))[0]
    _, domains = proof_mutate.parse(cs["entries"][cs["label_at"][label]][1])
    new_len = len(domains[d][0][first][2][proof_mutate.VECTORS.index(vec)])
    k = cases.item_op(cs["prog"], d, vec, 8 * new_len if d == 0 else new_len // 8)
    if k is None:
        return []
    return [[k - 1], [k], [k + 1], [k, k + 300, k + 900]]


def run_stream(rv, name, cs, monkeypatch, part):
    """part: "whole" (no cut, both modes; a malformed proof is refused here, at begin, before any piece is fed, so the other parts
    leave those entries out), "137_strict" / "137_compat" (a cut every 137 ops) or "boundary" (boundary_cuts, both modes).  WIDE
    runs every one of them a second time with the pieces compiled on the device."""
    rep = Report(f"{name} streaming verifier, {part}")
    prog, wc, n = cs["prog"], cs["wc"], len(cs["prog"])
    every137 = list(range(137, n, 137))
    modes = [m for m in MODES if part in ("whole", "boundary") or part == ("137_strict" if m[0] else "137_compat")]
    n_boundary = 0
    for i in cs["thin"]:
        label, p, want = cs["entries"][i][0], cs["proofs"][i], cs["answers"][i]
        if part == "whole":
            cut_sets = [[]]
        elif want[0] == MALFORMED:
            continue
        elif part == "boundary":
            cut_sets = boundary_cuts(cs, label)
            n_boundary += len(cut_sets)
        else:
            cut_sets = [every137]
        for cuts in cut_sets:
            for device in ((False, True) if name == "WIDE" else (False,)):
                for strict, k in modes:
                    rep.check(label, f"cuts {cuts[:4]}{' ...' if len(cuts) > 4 else ''}, strict={strict}, device compile={device}",
                              got(stream_verify, p, prog, wc, cuts, strict, device_compile=device), want[k])
    assert part != "boundary" or n_boundary >= 40, n_boundary
    rep.done()


# ---- 6. rv_verify_shard_groups + rv_verify_finish_ex
def run_groups(rv, name, cs, monkeypatch, world):
    from reverie_amd import ReverieError
    from reverie_amd.dist import HipShardBackend

    rep = Report(f"{name} rv_verify_shard_groups")
    c = cs["circuit"]
    be = HipShardBackend(c)
    ranks = lists("partition", world)
    for i in cs["thin"]:
        (label, data), p, want = cs["entries"][i], cs["proofs"][i], cs["answers"][i]
        if want[0] != MALFORMED:
            dig, zc, _ = verify_split(c, data, ranks)
            for strict, k in MODES:
                rep.check(label, f"world {world}, strict={strict}", finish(data, dig, 0 if strict else COMPAT, zc), want[k])
            continue
        # malformed: the rank that owns the altered group refuses the proof, the others do their part
        group = proof_mutate.split_label(label)[2]
        assert group is not None, label
        for r, groups in enumerate(ranks):
            try:
                be.verify_groups(p, groups)
                have = "ok"
            except ReverieError as e:
                have = ("err", e.code)
            rep.check(label, f"world {world}, rank {r} of groups {groups}", have, MALFORMED if group in groups else "ok")
    rep.done()


RUN = {
    "verify_ex": run_verify_ex, "verify_ops": run_verify_ops, "verify_batch": run_verify_batch,
    "stream_whole": lambda *a: run_stream(*a, "whole"), "stream_137_strict": lambda *a: run_stream(*a, "137_strict"),
    "stream_137_compat": lambda *a: run_stream(*a, "137_compat"), "stream_boundary": lambda *a: run_stream(*a, "boundary"),
    "stream_batch": lambda *a: run_stream_batch(*a, 0), "stream_batch_1024": lambda *a: run_stream_batch(*a, 1024),
    "groups_world2": lambda *a: run_groups(*a, 2), "groups_world8": lambda *a: run_groups(*a, 8),
}


@pytest.mark.parametrize("entry", list(RUN))
@pytest.mark.parametrize("name", cases.NAMES)
def test_altered_lengths(rv, case, monkeypatch, name, entry):
    RUN[entry](rv, name, case, monkeypatch)


# ---- the fused Z64 verifier's quad-group split: a proof of more than 4 MiB
SPLIT_TARGETS = (("r0", 0), ("r3", 0), ("all8", 4))  # (THINNED: the target axis; every Z64 length change is kept)
_split = {}


@pytest.mark.parametrize("vec", proof_mutate.VECTORS)
def test_z64_quad_group_split(rv, oracle, rule_seeds, monkeypatch, vec):
    """rv_verify_ex copies a proof with 4 MiB or more of online records on its second stream, and the fused Z64 verifier of a
    pure Z64 circuit then runs the quad groups without an opened repetition FIRST, the proof's copy and k_unpack64 beside them,
    and the first quad group's levels behind the supplied values (verify.inc: split64).  circuit Z is too small for that; this
    one is not, with any entry's lengths: the upload is computed and asserted for each.  Every Z64 length change of one vector
    per case, on record 0 and record 3 of group 0 and all eight records of group 4, with RV_Z64_FUSED_VERIFY unset and 0."""
    from reverie_amd import _lib
    from test_gpu_verify_groups import parse_records

    if not _split:
        prog, w64, wc = cases.split_circuit()
        good = oracle.prove(prog, [], w64, wc, rule_seeds)
        assert fused_eligible(rv, prog, wc, monkeypatch)
        _split.update(prog=prog, wc=wc, good=good, circuit=rv.Circuit(prog, wc))
        assert bytes(rv.Proof.new(_split["circuit"], [], w64, seeds=rule_seeds)) == good
    prog, wc, good, c = (_split[k] for k in ("prog", "wc", "good", "circuit"))
    assert not (prog["domain"] != 1).any()  # (the split is a pure Z64 circuit's)
    entries = list(proof_mutate.catalogue(good, targets=SPLIT_TARGETS, domains=("z64",), vectors=(vec,), same_length=False))
    assert len(entries) == len(SPLIT_TARGETS) * 15
    answers = cases.answers(oracle, prog, wc, entries)
    hook = _lib.lib().rv_hook_verify_proof_bytes
    rep = Report(f"SPLIT rv_verify_ex, {vec}")
    for env in ENV["Z"]:
        set_env(monkeypatch, env)
        assert rv.Proof(good).verify(c)
        for (label, data), want in zip(entries, answers):
            upload = sum(r[1] for dom in parse_records(data) for r in dom)  # the online records: what the verifier copies
            assert upload >= 4 << 20, (label, upload)
            p = rv.Proof(data)
            for strict, k in MODES:
                before = hook()
                rep.check(label, f"strict={strict} {env}", got(p.verify, c, strict=strict), want[k])
                assert hook() - before == upload, label
    assert {a[0] for a in answers} == {True, False}  # (no Z64 length is malformed)
    rep.done()
