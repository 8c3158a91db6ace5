"""Circuits compiled on the GPU with their wires' final values (RV_COMPILE_KEEP_WIRES | RV_COMPILE_DEVICE_KEEP_WIRES), from host
arrays and from torch GPU tensors: evaluations equal the host-compiled keep_wires circuit's and tests/eval_ref.py's model, proofs
are the host-compiled circuit's bytes, and the CLI's oneshot prints the same under --compiler device-b2a as under --compiler host.

The plain form of a program goes to the device compiler only when its K = 1 compile is final, which a program with one B2A (an
adder some 190 levels deep) is not: those are built with whole_prover=True here, and the plain form with B2A is covered by
test_gpu_compile_device_b2a.py's wide program (adders side by side)."""
import os
import subprocess
import sys

import numpy as np
import pytest

import eval_ref
from reverie_amd.ops import B2A, GF2, Z64, program
from test_gpu_compile_device_b2a import gen_b2a, wide_program
from test_gpu_compile_device_keep import gf2_hand_programs, mixed_hand_programs
from test_gpu_compile_device_z64 import _tensor, gen_mixed

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEVICE_KW = {"keep_wires": True, "device_compile": True, "device_z64": True, "device_b2a": True, "device_keep_wires": True}
TENSOR_KW = {"keep_wires": True, "device_z64": True, "device_b2a": True, "device_keep_wires": True}
BATCHES = (1, 32, 33)

_CASES = {}


def cases():
    """name -> (program, wire counts, whole_prover); no Random op"""
    if not _CASES:
        hand2, handm = gf2_hand_programs(), mixed_hand_programs()
        for name in ("unread_last_add", "overwritten_three_times", "constants_and_aliases", "sum_of_k_plus_1_rows", "wires_257_holes"):
            ops, wc = hand2[name]
            for wp in (False, True):
                _CASES["%s_%s" % (name, "lazy" if wp else "plain")] = (program(ops), wc, wp)
        for name in ("z64_overwritten", "no_gf2_wires"):
            ops, wc, _ = handm[name]
            _CASES[name + "_plain"] = (program(ops), wc, False)
        for name in ("b2a_last_writer", "b2a_destination_overwritten", "b2a_sources_overwritten"):
            ops, wc, _ = handm[name]
            _CASES[name + "_lazy"] = (program(ops), wc, True)
        rng = np.random.default_rng(0xE7A1)
        _CASES["random_mixed_plain"] = (gen_mixed(rng, 300, 12, 65, 0.5, randoms=False)[0], (12, 65), False)
        prog, _, _, wc = gen_b2a(rng, 300, 12, 100, 0.5, randoms=False)
        _CASES["random_mixed_b2a_lazy"] = (prog, wc, True)
        wide, wide_wc = wide_program(128)  # (final at K = 1: the plain form with B2A)
        _CASES["wide_b2a_plain"] = (wide, wide_wc, False)
    return _CASES


def witnesses(prog, batch, seed):
    rng = np.random.default_rng(seed)
    n2 = int(((prog["domain"] == 0) & (prog["opcode"] == 0)).sum())
    n64 = int(((prog["domain"] == 1) & (prog["opcode"] == 0)).sum())
    w64 = rng.integers(0, 1 << 63, (batch, n64), dtype=np.uint64) * np.uint64(2) + rng.integers(0, 2, (batch, n64), dtype=np.uint64)
    return rng.integers(0, 2, (batch, n2), dtype=np.uint8), w64


def _same(a, b, what):
    assert np.array_equal(a.ok, b.ok) and np.array_equal(a.n_failed, b.n_failed) and np.array_equal(a.first_failed_op, b.first_failed_op), what
    assert np.array_equal(a.gf2, b.gf2) and np.array_equal(a.z64, b.z64), what


@pytest.mark.parametrize("name", sorted(cases()))
def test_evaluations_equal_host_and_model(name):
    import reverie_amd

    prog, wc, wp = cases()[name]
    host = reverie_amd.Circuit(prog, wc, keep_wires=True, whole_prover=wp)
    dev = reverie_amd.Circuit(prog, wc, whole_prover=wp, **DEVICE_KW)
    ten = reverie_amd.Circuit.from_device_ops(_tensor(prog), wc, whole_prover=wp, **TENSOR_KW)
    try:
        assert not host.compiled_on_device and dev.compiled_on_device and ten.compiled_on_device
        for batch in BATCHES:
            w2, w64 = witnesses(prog, batch, 0xE7A100 + batch)
            ref2, ref64, ref_failed, ref_first = eval_ref.evaluate(prog, wc, w2, w64)
            want = host.evaluate_batch(w2, w64, values=True)
            assert np.array_equal(want.gf2, ref2) and np.array_equal(want.z64, ref64)
            assert np.array_equal(want.n_failed, ref_failed) and np.array_equal(want.first_failed_op, ref_first)
            for c in (dev, ten):
                _same(c.evaluate_batch(w2, w64, values=True), want, (name, batch))
        # one witness (rv_evaluate)
        w2, w64 = witnesses(prog, 1, 0xE7A1FF)
        want = host.evaluate(w2[0], w64[0])
        ref2, ref64, ref_failed, ref_first = eval_ref.evaluate(prog, wc, w2, w64)
        assert want.gf2.tolist() == ref2[0].tolist() and want.z64.tolist() == ref64[0].tolist() and want.n_failed == ref_failed[0]
        for c in (dev, ten):
            got = c.evaluate(w2[0], w64[0])
            assert (got.ok, got.n_failed, got.first_failed_op) == (want.ok, want.n_failed, want.first_failed_op), name
            assert np.array_equal(got.gf2, want.gf2) and np.array_equal(got.z64, want.z64), name
    finally:
        for c in (host, dev, ten):
            c.close()


def test_unread_final_sum_has_its_value():
    """the case the extra read is for: Add(w2, w0, w1) read by nothing -- wire 2 is a ^ b, not 0"""
    import reverie_amd

    prog = program([GF2.Input(0), GF2.Input(1), GF2.Add(2, 0, 1)])
    for wp in (False, True):
        c = reverie_amd.Circuit(prog, (0, 3), whole_prover=wp, **DEVICE_KW)
        assert c.compiled_on_device
        got = c.evaluate_batch(np.array([[0, 0], [0, 1], [1, 0], [1, 1]], np.uint8), values=True)
        assert got.gf2.tolist() == [[0, 0, 0], [0, 1, 1], [1, 0, 1], [1, 1, 0]]
        c.close()


def test_random_op_is_unsupported_as_on_the_host():
    import reverie_amd

    prog = program([GF2.Input(0), GF2.Random(1), GF2.Add(2, 0, 1), Z64.Random(0)])
    codes = []
    for kw in ({"keep_wires": True}, DEVICE_KW):
        c = reverie_amd.Circuit(prog, (1, 3), **kw)
        assert c.compiled_on_device == ("device_compile" in kw)
        with pytest.raises(reverie_amd.ReverieError) as e:
            c.evaluate([1])
        codes.append(e.value.code)
        c.close()
    assert codes == [8, 8]  # RV_E_UNSUPPORTED


@pytest.mark.parametrize("name", ["unread_last_add_plain", "sum_of_k_plus_1_rows_lazy", "z64_overwritten_plain", "b2a_last_writer_lazy", "random_valid_b2a_lazy"])
def test_proofs_are_the_host_circuits_bytes(rule_seeds, name):
    import reverie_amd

    if name == "random_valid_b2a_lazy":
        prog, w2, w64, wc = gen_b2a(np.random.default_rng(0xE7A2), 300, 12, 100, 0.5, valid=True)
        wp = True
    else:
        prog, wc, wp = cases()[name]
        w2, w64 = (w[0] for w in witnesses(prog, 1, 0xE7A2))
    host = reverie_amd.Circuit(prog, wc, keep_wires=True, whole_prover=wp)
    dev = reverie_amd.Circuit(prog, wc, whole_prover=wp, **DEVICE_KW)
    ten = reverie_amd.Circuit.from_device_ops(_tensor(prog), wc, whole_prover=wp, **TENSOR_KW)
    assert dev.compiled_on_device and ten.compiled_on_device
    for seeds in (rule_seeds, rule_seeds[::-1].copy()):
        want = bytes(reverie_amd.Proof.new(host, w2, w64, seeds=seeds))
        for c in (dev, ten):
            proof = reverie_amd.Proof.new(c, w2, w64, seeds=seeds)
            assert bytes(proof) == want, name
        assert reverie_amd.Proof(want).verify(dev, strict=True) and reverie_amd.Proof(want).verify(host, strict=True)
    for c in (host, dev, ten):
        c.close()


def test_cli_oneshot_device_compilers_print_what_host_prints(tmp_path, monkeypatch, capsys):
    """oneshot --evaluator gpu under every --compiler choice against --compiler host, for a witness that satisfies the program and
    one that does not: a shallow mixed program, which the device compiler takes, and one with a B2A, which it hands back in the plain
    form.  In this process for every choice, and for device-b2a on the first program in child processes.  First: the compile of the
    first program really runs on the GPU."""
    from reverie_amd import __main__ as cli
    from reverie_amd import proof

    shallow = [GF2.Input(0), GF2.Input(1), GF2.Mul(2, 0, 1), GF2.Add(3, 2, 0), GF2.AssertZero(3), Z64.Const(0, 5), Z64.Const(1, 6), Z64.Mul(2, 0, 1),
               Z64.SubConst(3, 2, 30), Z64.AssertZero(3)]
    adder = [GF2.Input(i) for i in range(64)] + [B2A(0, 0), Z64.Const(1, 5), Z64.Mul(2, 0, 1), Z64.SubConst(3, 2, 5 * 6), Z64.AssertZero(3)]
    made = []

    class Spy(proof.Circuit):
        def __init__(self, *a, **kw):
            super().__init__(*a, **kw)
            made.append(self.compiled_on_device)

    with monkeypatch.context() as m:
        m.setattr(proof, "Circuit", Spy)
        cli.evaluate_gpu(program(shallow), (4, 4), [0, 1], "device-b2a")
        cli.evaluate_gpu(program(shallow), (4, 4), [0, 1], "device")  # (Z64 ops without the Z64 bit: the host compiler's)
        cli.evaluate_gpu(program(shallow), (4, 4), [0, 1], "host")
    assert made == [True, False, False]

    def bits(x, n):
        return "\n".join(str((x >> i) & 1) for i in range(n)) + "\n"

    def run_here(compiler, prog_path, wit):  # -> (exit status, stdout, the SystemExit message or None)
        capsys.readouterr()
        try:
            status, msg = cli.main(["--operation", "oneshot", "--evaluator", "gpu", "--compiler", compiler, "--program-path", str(prog_path),
                                    "--witness-path", str(wit)]), None
        except SystemExit as e:
            status, msg = 1, str(e)
        return status, capsys.readouterr().out, msg

    env = dict(os.environ, PYTHONPATH=os.pathsep.join([ROOT] + [x for x in os.environ.get("PYTHONPATH", "").split(os.pathsep) if x]))

    def run_child(compiler, prog_path, wit):  # -> (exit status, stdout, stderr)
        r = subprocess.run([sys.executable, "-m", "reverie_amd", "--operation", "oneshot", "--evaluator", "gpu", "--compiler", compiler,
                            "--program-path", str(prog_path), "--witness-path", str(wit)], env=env, cwd=ROOT, capture_output=True, timeout=300)
        return r.returncode, r.stdout, r.stderr

    for tag, ops, good, bad in (("shallow", shallow, bits(2, 2), bits(1, 2)), ("adder", adder, bits(6, 64), bits(7, 64))):
        p = tmp_path / (tag + ".rvops")
        p.write_bytes(program(ops).tobytes())
        for text, ok in ((good, True), (bad, False)):
            wit = tmp_path / ("%s_%d.txt" % (tag, ok))
            wit.write_text(text)
            want = run_here("host", p, wit)
            assert (want[0] == 0) == ok and want[1].startswith("Evaluating program in cleartext"), (tag, ok, want)
            assert ok or "op %d" % (4 if tag == "shallow" else len(ops) - 1) in want[2]
            for compiler in ("device", "device-z64", "device-b2a"):
                assert run_here(compiler, p, wit) == want, (tag, compiler, ok)
            if tag == "shallow":  # the command line itself, byte for byte: standard output, standard error and the exit status
                want = run_child("host", p, wit)
                assert (want[0] == 0) == ok and want[1].startswith(b"Evaluating program in cleartext"), (ok, want)
                assert run_child("device-b2a", p, wit) == want, ok
