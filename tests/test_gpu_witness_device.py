"""Witnesses taken from device memory (rv_prove_wdev, rv_prove_device_wdev, rv_prove_batch_wdev, rv_prove_batch_device_wdev) and
evaluation that leaves its results there (rv_evaluate_batch_device), through the C-ABI and through the Python entry points that
take torch GPU tensors.

The yardstick is always the unchanged host-witness entry point on the same bytes: proofs are equal byte for byte, statuses and
values are rv_evaluate_batch's at the selected columns (tests/eval_ref.py is a second yardstick for the evaluator).  The device
witnesses are awkward on purpose: the GF(2) pointer is odd, the Z64 pointer sits at 8 but not 16 bytes, every witness is longer
than the Input ops consume (the surplus is 0xFF), and the rows of a batch are a stride apart whose padding is 0xFF too.
rv_hook_witness_traffic says that no witness byte went host-to-device and no result byte device-to-host.

Prover statements are satisfied by construction (golden circuits with their golden witness, random_gf2(p_assert=0)); the
evaluator's witnesses are random, with the generator's own witness planted in every third row, so that some hold and some fail."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import circuits
import eval_ref
from conftest import ROOT
from reverie_amd.ops import OP_ADD, OP_DTYPE, OP_INPUT, OP_RANDOM
from test_gpu_verify_device import golden

pytestmark = pytest.mark.gpu

NAMES = ("gf2_mix", "z64_mix", "sizehint_mixed", "adder64", "empty", "ref_test")
E_INVALID, E_SHORT, E_WIRE_OOB, E_UNSUPPORTED, E_ARG = 1, 2, 3, 8, 9


@pytest.fixture(scope="module")
def rv():
    import reverie_amd

    reverie_amd.Context.default()
    return reverie_amd


def lib():
    from reverie_amd import _lib

    return _lib.lib()


def traffic():
    """(witness bytes host-to-device, witness bytes taken from device memory, evaluation result bytes device-to-host)"""
    out = (C.c_uint64 * 3)()
    assert lib().rv_hook_witness_traffic(out) == 0
    return tuple(int(x) for x in out)


def schedules():
    out = (C.c_uint64 * 2)()
    assert lib().rv_hook_eval_schedules(out) == 0
    return int(out[0]), int(out[1])


def consumed(circuit):
    """witness bytes one statement of the circuit consumes"""
    info = circuit.info
    return info["gf2_inputs"] + 8 * info["z64_inputs"]


class DeviceWitness:
    """`B` witnesses in GPU memory and the same bytes on the host.  tg: uint8 [B][n2] at an odd address, tz: int64 [B][n64] at
    8 mod 16; n2 / n64 exceed the given witnesses by `surplus` elements of 0xFF bytes; the rows are `slack` elements further apart
    than they are long, the padding 0xFF as well.  hg / hz: packed host copies of the rows (surplus included)."""

    def __init__(self, g, z=None, surplus=(3, 2), slack=(5, 3)):
        import torch

        g = np.atleast_2d(np.asarray(g, np.uint8))
        B = g.shape[0]
        z = np.zeros((B, 0), np.uint64) if z is None else np.atleast_2d(np.asarray(z, np.uint64))
        assert z.shape[0] == B
        self.B = B
        self.n2, self.n64 = g.shape[1] + surplus[0], z.shape[1] + surplus[1]
        self.s2, self.s64 = self.n2 + slack[0], self.n64 + slack[1]
        self.buf2 = torch.full((1 + B * self.s2,), 0xFF, dtype=torch.uint8, device="cuda")
        rows2 = self.buf2[1:].view(B, self.s2)
        if g.shape[1]:
            rows2[:, :g.shape[1]] = torch.from_numpy(np.ascontiguousarray(g)).cuda()
        self.buf64 = torch.full((1 + B * self.s64,), -1, dtype=torch.int64, device="cuda")
        rows64 = self.buf64[1:].view(B, self.s64)
        if z.shape[1]:
            rows64[:, :z.shape[1]] = torch.from_numpy(np.ascontiguousarray(z).view(np.int64)).cuda()
        self.tg, self.tz = rows2[:, :self.n2], rows64[:, :self.n64]
        assert self.tg.data_ptr() % 2 == 1 and self.tz.data_ptr() % 16 == 8
        self.hg = np.ascontiguousarray(self.tg.cpu().numpy())
        self.hz = np.ascontiguousarray(self.tz.cpu().numpy()).view(np.uint64)
        torch.cuda.synchronize()

    def desc(self, **over):
        """the rv_dev_witness of these tensors (over: fields to falsify)"""
        from reverie_amd import _lib

        f = dict(gf2=self.tg.data_ptr(), n_gf2=self.n2, stride_gf2=self.s2, z64=self.tz.data_ptr(), n_z64=self.n64, stride_z64=self.s64)
        f.update(over)
        return _lib.DevWitness(**f)


def batch_seeds(rule_seeds, B):
    return np.stack([np.roll(rule_seeds, b, axis=0) ^ np.uint8(b) for b in range(B)]).astype(np.uint8)


_circuits = {}


@pytest.fixture
def gold(rv, name):
    if name not in _circuits:
        prog, w2, w64, wc, proof = golden(name)
        _circuits[name] = dict(circuit=rv.Circuit(prog, wc), w2=w2, w64=w64, proof=proof)
    return _circuits[name]


def framed(rv, dp):
    return bytes(dp.to_proof())


# ---------------------------------------------------------------- 1. single proofs
@pytest.mark.parametrize("name", NAMES)
def test_single_proofs(rv, rule_seeds, gold, name):
    c = gold["circuit"]
    W = DeviceWitness(gold["w2"], gold["w64"])
    want = bytes(rv.Proof.new(c, W.hg[0], W.hz[0], seeds=rule_seeds))
    assert want == gold["proof"]
    assert bytes(rv.DeviceProof.new(c, W.hg[0], W.hz[0], seeds=rule_seeds).to_proof()) == want
    t0 = traffic()
    assert bytes(rv.Proof.new(c, W.tg[0], W.tz[0], seeds=rule_seeds)) == want  # rv_prove_wdev
    t1 = traffic()
    assert (t1[0] - t0[0], t1[1] - t0[1], t1[2] - t0[2]) == (0, consumed(c), 0)
    assert framed(rv, rv.DeviceProof.new(c, W.tg[0], W.tz[0], seeds=rule_seeds)) == want  # rv_prove_device_wdev + rv_assemble_proof
    t2 = traffic()
    assert (t2[0] - t1[0], t2[1] - t1[1], t2[2] - t1[2]) == (0, consumed(c), 0)


def test_single_proof_random_gf2(rv, rule_seeds):
    prog, wit, wc = circuits.random_gf2(np.random.default_rng(21), p_assert=0)
    c = rv.Circuit(prog, wc)
    W = DeviceWitness(wit)
    want = bytes(rv.Proof.new(c, W.hg[0], [], seeds=rule_seeds))
    t0 = traffic()
    assert bytes(rv.Proof.new(c, W.tg[0], None, seeds=rule_seeds)) == want
    assert framed(rv, rv.DeviceProof.new(c, W.tg[0], None, seeds=rule_seeds)) == want
    t1 = traffic()
    assert t1[0] == t0[0] and t1[1] - t0[1] == 2 * consumed(c)


def test_witness_beyond_the_input_stage(rv, rule_seeds):
    """2^20 Input ops and 64 XORs: the witness no longer fits beside the seeds in the 1 MiB input stage, so the commitment takes its
    separate-allocation branch"""
    n = 1 << 20
    ops = np.zeros(n + 64, OP_DTYPE)
    ops["opcode"][:n] = OP_INPUT
    ops["dst"][:n] = np.arange(n, dtype=np.uint32)
    ops["opcode"][n:] = OP_ADD
    ops["dst"][n:] = np.arange(n, n + 64, dtype=np.uint32)
    ops["a"][n:] = np.arange(64, dtype=np.uint32)
    ops["b"][n:] = np.arange(1, 65, dtype=np.uint32) * 1000
    c = rv.Circuit(ops, (0, n + 64))
    try:
        assert consumed(c) == n
        W = DeviceWitness(np.random.default_rng(3).integers(0, 2, n).astype(np.uint8))
        want = bytes(rv.Proof.new(c, W.hg[0], [], seeds=rule_seeds))
        t0 = traffic()
        assert bytes(rv.Proof.new(c, W.tg[0], None, seeds=rule_seeds)) == want
        assert framed(rv, rv.DeviceProof.new(c, W.tg[0], None, seeds=rule_seeds)) == want
        t1 = traffic()
        assert t1[0] == t0[0] and t1[1] - t0[1] == 2 * n
    finally:
        c.close()


@pytest.mark.parametrize("name", ("adder64",))
def test_flipped_bit_is_an_invalid_witness(rv, rule_seeds, gold, name):
    c = gold["circuit"]
    w2 = np.asarray(gold["w2"], np.uint8).copy()
    w2[0] ^= 1
    W = DeviceWitness(w2, gold["w64"])
    for fn in (rv.Proof.new, rv.DeviceProof.new):
        for g, z in ((W.hg[0], W.hz[0]), (W.tg[0], W.tz[0])):  # (the sibling first: the same code)
            with pytest.raises(rv.ReverieError) as e:
                fn(c, g, z, seeds=rule_seeds)
            assert e.value.code == E_INVALID


# ---------------------------------------------------------------- 2. batches
def host_batch(rv, c, W, seeds):
    return [bytes(p) for p in rv.Proof.new_batch(c, W.hg, W.hz, seeds=seeds)]


def host_batch_device(rv, c, W, seeds):
    return [dp.tensor.cpu().numpy().tobytes() for dp in rv.prove_batch_device(c, W.hg, W.hz, seeds=seeds)]


def device_batches(rv, c, W, seeds):
    """(rv_prove_batch_wdev's proofs, rv_prove_batch_device_wdev's), with the traffic of the two calls checked"""
    t0 = traffic()
    a = [bytes(p) for p in rv.Proof.new_batch(c, W.tg, W.tz, seeds=seeds)]
    b = [dp.tensor.cpu().numpy().tobytes() for dp in rv.prove_batch_device(c, W.tg, W.tz, seeds=seeds)]
    t1 = traffic()
    assert (t1[0] - t0[0], t1[1] - t0[1], t1[2] - t0[2]) == (0, 2 * W.B * consumed(c), 0)
    return a, b


@pytest.mark.parametrize("B", (3, 5))
@pytest.mark.parametrize("name", ("gf2_mix", "z64_mix", "sizehint_mixed"))
def test_batches(rv, rule_seeds, gold, name, B):
    c = gold["circuit"]
    W = DeviceWitness(np.tile(np.asarray(gold["w2"], np.uint8), (B, 1)), np.tile(np.asarray(gold["w64"], np.uint64), (B, 1)))
    assert W.tg.stride(0) > W.tg.shape[1] and W.tz.stride(0) > W.tz.shape[1]
    seeds = batch_seeds(rule_seeds, B)
    want = host_batch(rv, c, W, seeds)
    assert want[0] == gold["proof"] and len(set(want)) == B and host_batch_device(rv, c, W, seeds) == want
    a, b = device_batches(rv, c, W, seeds)
    assert a == want and b == want


@pytest.mark.parametrize("name", ("z64_mix",))
def test_batch_chunks(rv, rule_seeds, gold, monkeypatch, name):
    """RV_BATCH_MAX=2, five statements: chunks of 2, 2 and 1, the later ones' witnesses a whole number of strides in"""
    c = gold["circuit"]
    B = 5
    W = DeviceWitness(np.tile(np.asarray(gold["w2"], np.uint8), (B, 1)), np.tile(np.asarray(gold["w64"], np.uint64), (B, 1)))
    seeds = batch_seeds(rule_seeds, B)
    want = host_batch(rv, c, W, seeds)
    monkeypatch.setenv("RV_BATCH_MAX", "2")
    assert host_batch(rv, c, W, seeds) == want
    a, b = device_batches(rv, c, W, seeds)
    assert a == want and b == want


CHILD = r"""
import sys
import numpy as np
sys.path[:0] = [{root!r}, {tests!r}]
import reverie_amd as rv
from test_gpu_verify_device import golden
from test_gpu_witness_device import DeviceWitness, traffic, consumed
prog, w2, w64, wc, proof = golden("gf2_mix")
c = rv.Circuit(prog, wc)
seeds = np.frombuffer(bytes.fromhex(sys.argv[1]), np.uint8).reshape(2, 256, 16)
W = DeviceWitness(np.tile(np.asarray(w2, np.uint8), (2, 1)))
want = [bytes(rv.Proof.new(c, w2, w64, seeds=seeds[b])) for b in range(2)]
assert want[0] == proof
assert [bytes(p) for p in rv.Proof.new_batch(c, W.hg, None, seeds=seeds)] == want, "host witnesses, worker threads"
t0 = traffic()
have = [bytes(p) for p in rv.Proof.new_batch(c, W.tg, None, seeds=seeds)]
assert have == want, "device witnesses, worker threads: bytes differ"
have = [dp.tensor.cpu().numpy().tobytes() for dp in rv.prove_batch_device(c, W.tg, None, seeds=seeds)]
assert have == want, "device witnesses, proof after proof: bytes differ"
t1 = traffic()
assert t1[0] == t0[0] and t1[1] - t0[1] == 4 * consumed(c) and t1[2] == t0[2], (t0, t1)
print("child ok")
"""


def test_large_circuit_branches(rule_seeds):
    """RV_BATCH_BIG_GATES is read once per process: in a fresh child gf2_mix counts as a large circuit, so rv_prove_batch_wdev
    goes through the worker threads and rv_prove_batch_device_wdev proves one statement after the other"""
    seeds = np.stack([rule_seeds, rule_seeds[::-1]]).astype(np.uint8)
    env = dict(os.environ, RV_BATCH_BIG_GATES="1")
    code = CHILD.format(root=ROOT, tests=os.path.join(ROOT, "tests"))
    r = subprocess.run([sys.executable, "-c", code, seeds.tobytes().hex()], env=env, cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "child ok" in r.stdout, r.stdout + r.stderr


# ---------------------------------------------------------------- 3. evaluation
def without_random(prog):
    """the program without its Random ops (the evaluator refuses them; the generators never assert a wire that depends on one, so
    their own witness still satisfies what is left)"""
    return np.ascontiguousarray(prog[~((prog["opcode"] == OP_RANDOM) & (prog["domain"] <= 1))])


def never_written(prog, domain, n_wires):
    """the last wire of the domain that no op writes"""
    written = set(int(d) for d in prog["dst"][prog["domain"] == domain])
    if domain == 1:
        written |= set(int(d) for d in prog["dst"][prog["domain"] == 2])  # (B2A writes a Z64 wire)
    return max(w for w in range(n_wires) if w not in written)


_eval = {}


def eval_case(rv, kind):
    """circuit, program, wire counts (with spare wires nothing writes), the generator's witness"""
    if kind not in _eval:
        if kind == "gf2":
            prog, w2, _wc = circuits.random_gf2(np.random.default_rng(3), n_in=12, n_gates=300, n_wires=40)
            w64, wc = [], (0, 44)
        else:
            prog, w2, w64, _wc = circuits.random_mixed(np.random.default_rng(2))
            wc = (14, 93)
        prog = without_random(prog)
        _eval[kind] = dict(circuit=rv.Circuit(prog, wc, keep_wires=True), prog=prog, wc=wc, w2=np.asarray(w2, np.uint8),
                           w64=np.asarray(w64, np.uint64), refs={})
    return _eval[kind]


def eval_witnesses(case, B, slack):
    """random witnesses, the generator's own in every third row; the device form, and rv_evaluate_batch's answer on the same
    bytes (computed once per shape and left alone)"""
    key = (B, slack)
    if key not in case["refs"]:
        rng = np.random.default_rng(100 + B)
        g = rng.integers(0, 2, (B, len(case["w2"]))).astype(np.uint8)
        z = rng.integers(0, 1 << 63, (B, len(case["w64"])), dtype=np.uint64)
        g[::3], z[::3] = case["w2"], case["w64"]
        W = DeviceWitness(g, z, slack=slack)
        case["refs"][key] = (W, case["circuit"].evaluate_batch(W.hg, W.hz, values=True))
    return case["refs"][key]


def check_device_evaluation(case, W, ref, env_note=""):
    """every selection (none, every wire, repeats out of order, a wire nothing writes, an empty list) against the host call's columns"""
    c, prog, (n64, n2) = case["circuit"], case["prog"], case["wc"]
    want_status = np.stack([ref.n_failed, ref.first_failed_op], axis=1).astype(np.int64)
    dead2 = never_written(prog, 0, n2)
    sels2 = [None, ..., [n2 - 1, 0, 0, n2 - 1], [dead2], []]
    if n64:
        dead64 = never_written(prog, 1, n64)
        sels64 = [None, ..., [n64 - 1, 0, 0, n64 - 1], [dead64], []]
    else:
        sels64 = [None, None, None, ..., []]
    t0, n_calls = traffic(), 0
    for s2, s64 in zip(sels2, sels64):
        r = c.evaluate_batch_device(W.tg, W.tz, gf2_wires=s2, z64_wires=s64)
        n_calls += 1
        assert np.array_equal(r.status.cpu().numpy(), want_status), (env_note, s2)
        assert np.array_equal(r.n_failed.cpu().numpy(), ref.n_failed) and np.array_equal(r.ok.cpu().numpy(), ref.ok)
        assert np.array_equal(r.first_failed_op.cpu().numpy(), ref.first_failed_op)
        for have, sel, full in ((r.gf2, s2, ref.gf2), (r.z64, s64, ref.z64)):
            if sel is None:
                assert have is None
                continue
            have = have.cpu().numpy()
            if full.dtype == np.uint64:
                have = have.view(np.uint64)
            want = full if sel is Ellipsis else full[:, sel]
            assert have.shape == want.shape and np.array_equal(have, want), (env_note, sel)
        if s2 == [dead2]:
            assert not r.gf2.any()
    t1 = traffic()
    assert (t1[0] - t0[0], t1[1] - t0[1], t1[2] - t0[2]) == (0, n_calls * W.B * consumed(c), 0)


MODES = {"plain": ({}, (0, 0)), "part32": ({"RV_EVAL_PART": "32"}, (0, 0)), "poison": ({"RV_EVAL_POISON": "1"}, (0, 0)),
         "strided": ({}, (5, 3)), "strided_part32_poison": ({"RV_EVAL_PART": "32", "RV_EVAL_POISON": "1"}, (5, 3))}


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("B", (1, 31, 32, 33, 65))
@pytest.mark.parametrize("kind", ("gf2", "mixed"))
def test_evaluation(rv, monkeypatch, kind, B, mode):
    case = eval_case(rv, kind)
    env, slack = MODES[mode]
    W, ref = eval_witnesses(case, B, slack)  # (the host call ran without the knobs: whole batch, no poison)
    assert (W.tg.stride(0) > W.tg.shape[1]) == bool(slack[0]) or B == 1
    if B >= 31:
        assert (ref.n_failed > 0).any() and (ref.n_failed == 0).any()
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    s0 = schedules()
    check_device_evaluation(case, W, ref, mode)
    s1 = schedules()
    assert s1[1] > s0[1] and s1[0] == s0[0]  # (these circuits are walked)
    if "RV_EVAL_PART" in env and B == 65:
        assert s1[1] - s0[1] == 5 * 3  # three parts per call


@pytest.mark.parametrize("kind", ("gf2", "mixed"))
def test_evaluation_equals_the_reference_model(rv, kind):
    case = eval_case(rv, kind)
    W, ref = eval_witnesses(case, 33, (5, 3))
    n_in2, n_in64 = len(case["w2"]), len(case["w64"])
    g, z, nf, ff = eval_ref.evaluate(case["prog"], case["wc"], W.hg[:, :n_in2], W.hz[:, :n_in64] if n_in64 else None)
    r = case["circuit"].evaluate_batch_device(W.tg, W.tz, gf2_wires=..., z64_wires=... if case["wc"][0] else None)
    assert np.array_equal(r.n_failed.cpu().numpy(), nf) and np.array_equal(r.first_failed_op.cpu().numpy(), ff)
    assert np.array_equal(r.gf2.cpu().numpy(), g)
    if case["wc"][0]:
        assert np.array_equal(r.z64.cpu().numpy().view(np.uint64), z)
    assert (nf > 0).any() and (nf == 0).any()


def test_evaluation_level_by_level(rv):
    """a wide, shallow circuit runs one launch per level (schedule (a)); the small ones above are walked (schedule (b)): the device
    form gives the host form's answers on both"""
    prog, wit, wc, _st = circuits.layered_gf2(n_in=512, width=16384, layers=3, seed=3)
    c = rv.Circuit(prog, wc, keep_wires=True)
    try:
        rng = np.random.default_rng(8)
        g = rng.integers(0, 2, (33, 512)).astype(np.uint8)
        g[::3] = wit
        W = DeviceWitness(g)
        ref = c.evaluate_batch(W.hg, None, values=True)
        assert (ref.n_failed > 0).any() and (ref.n_failed == 0).any()
        s0 = schedules()
        last = wc[1] - 1
        t0 = traffic()
        for sel in (..., [last, 0, 0, last], []):
            r = c.evaluate_batch_device(W.tg, None, gf2_wires=sel)
            assert np.array_equal(r.n_failed.cpu().numpy(), ref.n_failed) and np.array_equal(r.first_failed_op.cpu().numpy(), ref.first_failed_op)
            assert np.array_equal(r.gf2.cpu().numpy(), ref.gf2 if sel is Ellipsis else ref.gf2[:, sel])
        s1 = schedules()
        assert s1[0] - s0[0] == 3 and s1[1] == s0[1]
        t1 = traffic()
        assert t1[0] == t0[0] and t1[2] == t0[2]
    finally:
        c.close()


# ---------------------------------------------------------------- 4. refusals
def test_refusals(rv, rule_seeds):
    import torch

    from reverie_amd import _lib

    L = lib()
    # a GF(2) circuit for the provers, a Z64 one for the alignment rule, the evaluator's circuits
    prog, w2, w64, wc, _proof = golden("gf2_mix")
    c2 = rv.Circuit(prog, wc)
    progz, w2z, w64z, wcz, _ = golden("z64_mix")
    cz = rv.Circuit(progz, wcz)
    ev = eval_case(rv, "gf2")
    ce = ev["circuit"]
    plain = rv.Circuit(ev["prog"], ev["wc"])  # (no keep_wires)
    rnd_prog, rnd_wit, rnd_wc = circuits.random_gf2(np.random.default_rng(1), n_in=12, n_gates=300, n_wires=40)
    assert (rnd_prog["opcode"] == OP_RANDOM).any()
    crnd = rv.Circuit(rnd_prog, rnd_wc)
    try:
        W2 = DeviceWitness(np.tile(np.asarray(w2, np.uint8), (2, 1)))
        Wz = DeviceWitness(np.tile(np.asarray(w2z, np.uint8), (2, 1)), np.tile(np.asarray(w64z, np.uint64), (2, 1)))
        We = DeviceWitness(np.tile(ev["w2"], (2, 1)))
        Wr = DeviceWitness(np.tile(np.asarray(rnd_wit, np.uint8), (2, 1)))
        seeds = batch_seeds(rule_seeds, 2)
        sp = seeds.ctypes.data_as(C.c_void_p)
        n_wires2 = ev["wc"][1]
        proof, n = C.c_void_p(), C.c_size_t()
        proofs, lens = (C.c_void_p * 2)(), (C.c_size_t * 2)()
        comm, omit, lens4 = (C.c_uint8 * 32)(), (C.c_uint8 * 256)(), (C.c_size_t * 4)()

        def proof_len(c):
            sz2, sz64 = c.record_sizes()
            return 64 + 40 * (sz2 + sz64) + 2 * 216 * 48

        def stride_of(c):
            return (proof_len(c) + 255) & ~255

        total = proof_len(c2)
        dst = torch.full((2 * max(stride_of(c2), stride_of(cz)) + 512,), 0xA5, dtype=torch.uint8, device="cuda")
        status = torch.full((2, 2), 7, dtype=torch.int64, device="cuda")
        vals = torch.full((2, n_wires2), 7, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()

        def prove(c, d):
            return L.rv_prove_wdev(c.ctx.handle, c.handle, C.byref(d), sp, C.byref(proof), C.byref(n))

        def prove_device(c, d):
            return L.rv_prove_device_wdev(c.ctx.handle, c.handle, C.byref(d), sp, C.c_void_p(dst.data_ptr()), comm, omit, lens4)

        def prove_batch(c, d):
            return L.rv_prove_batch_wdev(c.ctx.handle, c.handle, 2, C.byref(d), sp, proofs, lens)

        def prove_batch_device(c, d, at=None):
            return L.rv_prove_batch_device_wdev(c.ctx.handle, c.handle, 2, C.byref(d), sp, C.c_void_p(dst.data_ptr() if at is None else at),
                                                stride_of(c), C.byref(n))

        def evaluate(c, d, sel=None, n_sel=0, values=None):
            selp = (C.c_uint32 * max(len(sel), 1))(*sel) if sel is not None else None
            return L.rv_evaluate_batch_device(c.ctx.handle, c.handle, 2, C.byref(d), selp, n_sel, None, 0,
                                              C.c_void_p(values.data_ptr()) if values is not None else None, None, C.c_void_p(status.data_ptr()))

        every = (prove, prove_device, prove_batch, prove_batch_device)
        t0, s0 = traffic(), schedules()
        # host memory named as device memory
        host = np.zeros(4096, np.uint8)
        for fn in every:
            assert fn(c2, W2.desc(gf2=host.ctypes.data)) == E_ARG, fn.__name__
        assert evaluate(ce, We.desc(gf2=host.ctypes.data)) == E_ARG
        # a Z64 pointer at an odd multiple of 4
        assert (Wz.tz.data_ptr() + 4) % 8 == 4
        for fn in every:
            assert fn(cz, Wz.desc(z64=Wz.tz.data_ptr() + 4)) == E_ARG, fn.__name__
        # rows that overlap: a stride smaller than the witness
        for fn in (prove_batch, prove_batch_device):
            assert fn(c2, W2.desc(stride_gf2=W2.n2 - 1)) == E_ARG, fn.__name__
        assert evaluate(ce, We.desc(stride_gf2=We.n2 - 1)) == E_ARG
        # a witness one short of the Input ops
        n_in = c2.info["gf2_inputs"]
        assert n_in > 0
        for fn in every:
            assert fn(c2, W2.desc(n_gf2=n_in - 1, stride_gf2=W2.s2)) == E_SHORT, fn.__name__
        assert evaluate(ce, We.desc(n_gf2=ce.info["gf2_inputs"] - 1)) == E_SHORT
        # the witness inside the destination
        inside = _lib.DevWitness(gf2=dst.data_ptr() + 257, n_gf2=W2.n2, stride_gf2=W2.s2)
        assert prove_batch_device(c2, inside) == E_ARG and prove_device(c2, inside) == E_ARG
        over_status = _lib.DevWitness(gf2=status.data_ptr() + 1, n_gf2=We.n2, stride_gf2=We.n2)
        assert evaluate(ce, over_status) == E_ARG
        # a wire index at the wire count; values of a circuit without keep_wires; a Random op
        assert evaluate(ce, We.desc(), sel=[0, n_wires2], n_sel=2, values=vals) == E_WIRE_OOB
        assert evaluate(plain, We.desc(), values=vals) == E_ARG
        assert evaluate(crnd, Wr.desc()) == E_UNSUPPORTED
        # sel NULL with a count
        assert L.rv_evaluate_batch_device(ce.ctx.handle, ce.handle, 2, C.byref(We.desc()), None, 2, None, 0, C.c_void_p(vals.data_ptr()), None,
                                          C.c_void_p(status.data_ptr())) == E_ARG
        # misaligned outputs
        assert L.rv_evaluate_batch_device(ce.ctx.handle, ce.handle, 2, C.byref(We.desc()), None, 0, None, 0, None, None,
                                          C.c_void_p(status.data_ptr() + 8)) == E_ARG
        assert traffic() == t0 and schedules() == s0, "a refused call ran something"
        torch.cuda.synchronize()
        assert bool((dst == 0xA5).all()) and bool((status == 7).all()) and bool((vals == 7).all()), "a refused call wrote"
        # ... and the same calls with nothing falsified are taken
        assert prove_batch_device(c2, W2.desc()) == 0 and n.value == total
        assert evaluate(ce, We.desc(), sel=[0, n_wires2 - 1], n_sel=2, values=vals) == 0
        assert evaluate(plain, We.desc()) == 0
        assert traffic()[1] > t0[1]
    finally:
        for c in (c2, cz, plain, crnd):
            c.close()


# ---------------------------------------------------------------- 5. Python
def test_python_entry_points(rv, rule_seeds):
    import torch

    prog, w2, w64, wc, proof = golden("sizehint_mixed")
    c = rv.Circuit(prog, wc)
    try:
        g = np.asarray(w2, np.uint8)
        z = np.asarray(w64, np.uint64)
        tg, tz = torch.from_numpy(g).cuda(), torch.from_numpy(z.view(np.int64)).cuda()
        tb = tg.to(torch.bool)
        assert bytes(rv.Proof.new(c, g, z, seeds=rule_seeds)) == proof
        assert bytes(rv.Proof.new(c, tg, tz, seeds=rule_seeds)) == proof
        assert bytes(rv.Proof.new(c, tb, tz, seeds=rule_seeds)) == proof
        assert bytes(rv.Proof.new(prog, tg, tz, wc, seeds=rule_seeds)) == proof  # (a raw op list is compiled first)
        assert bytes(rv.DeviceProof.new(c, tg, tz, seeds=rule_seeds).to_proof()) == proof
        seeds = batch_seeds(rule_seeds, 3)
        gB, zB = np.tile(g, (3, 1)), np.tile(z, (3, 1))
        tgB, tzB = torch.from_numpy(gB).cuda(), torch.from_numpy(zB.view(np.int64)).cuda()
        want = [bytes(p) for p in rv.Proof.new_batch(c, gB, zB, seeds=seeds)]
        assert [bytes(p) for p in rv.Proof.new_batch(c, tgB, tzB, seeds=seeds)] == want
        assert [dp.tensor.cpu().numpy().tobytes() for dp in rv.prove_batch_device(c, tgB, tzB, seeds=seeds)] == want
        assert rv.verify_batch_device(c, rv.prove_batch_device(c, tgB, tzB)) == [True] * 3  # (seeds from the OS)
        if hasattr(torch, "uint64"):
            tu = torch.from_numpy(zB.view(np.int64)).cuda().view(torch.uint64)
            assert [bytes(p) for p in rv.Proof.new_batch(c, tgB, tu, seeds=seeds)] == want
        with pytest.raises(TypeError):
            rv.Proof.new(c, tg, z, seeds=rule_seeds)
        with pytest.raises(ValueError):
            rv.Proof.new_batch(c, tgB.to(torch.int32), tzB, seeds=seeds)
    finally:
        c.close()
    # the evaluator
    case = eval_case(rv, "mixed")
    W, ref = eval_witnesses(case, 33, (5, 3))
    ce = case["circuit"]
    r = ce.evaluate_batch_device(W.tg, W.tz, gf2_wires=[5, 3, 5], z64_wires=np.array([2, 0]))
    assert isinstance(r, rv.DeviceEvaluation) and r.status.device.type == "cuda" and r.status.dtype == torch.int64
    assert r.gf2.dtype == torch.uint8 and r.z64.dtype == torch.int64 and tuple(r.gf2.shape) == (33, 3) and tuple(r.z64.shape) == (33, 2)
    assert np.array_equal(r.gf2.cpu().numpy(), ref.gf2[:, [5, 3, 5]]) and np.array_equal(r.z64.cpu().numpy().view(np.uint64), ref.z64[:, [2, 0]])
    assert np.array_equal(r.ok.cpu().numpy(), ref.ok) and np.array_equal(r.first_failed_op.cpu().numpy(), ref.first_failed_op)
    assert r.n_failed.data_ptr() == r.status.data_ptr()  # (views of the status records)
    none = ce.evaluate_batch_device(W.tg, W.tz)
    assert none.gf2 is None and none.z64 is None and np.array_equal(none.n_failed.cpu().numpy(), ref.n_failed)
    with pytest.raises(TypeError):
        ce.evaluate_batch_device(W.tg.cpu(), W.tz.cpu())
    with pytest.raises(rv.ReverieError) as e:
        ce.evaluate_batch_device(W.tg, W.tz, gf2_wires=[case["wc"][1]])
    assert e.value.code == E_WIRE_OOB
