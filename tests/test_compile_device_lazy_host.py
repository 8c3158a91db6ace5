"""The corpus of test_gpu_compile_device_lazy.py on the host compiler alone: the GPU comparison means something only if the programs
exercise the lazy-sum rule both ways -- sums that stay symbolic under RV_COMPILE_WHOLE_PROVER and sums that are materialised.  These
shares are conditions on the inputs (lazy_corpus.py), not measurements.  Also: the getter that tells which compiler made a circuit
is declared and exported."""
import os
import re

import lazy_corpus
from lazy_corpus import RV_COMPILE_WHOLE_PROVER

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _both(prog, wc, monkeypatch):
    with monkeypatch.context() as m:
        m.setenv("RV_LAZY_K", "1")
        rc1, k1 = lazy_corpus.compile_info(prog, wc, 0)
    rc3, k3 = lazy_corpus.compile_info(prog, wc, RV_COMPILE_WHOLE_PROVER)
    assert rc1 == 0 and rc3 == 0
    return k1, k3


def test_random_corpus_exercises_the_rule(monkeypatch):
    monkeypatch.delenv("RV_LAZY_K", raising=False)
    progs = lazy_corpus.random_programs()
    assert len(progs) == 240
    fewer = some = written = 0
    for prog, wit, wc in progs:
        k1, k3 = _both(prog, wc, monkeypatch)
        assert k3.gf2_linear <= k1.gf2_linear
        assert (k3.gf2_inputs, k3.gf2_muls, k3.gf2_asserts, k3.gf2_masks) == (k1.gf2_inputs, k1.gf2_muls, k1.gf2_asserts, k1.gf2_masks)
        fewer += k3.gf2_linear < k1.gf2_linear
        some += k3.gf2_linear > 0
        written += k3.gf2_rows_written > 0
    print("sums stay symbolic on", fewer, "programs; linear gates on", some, "; sums materialised on", written)
    assert 2 * fewer >= len(progs), fewer      # sums really stay symbolic
    assert 4 * some >= len(progs), some        # ... and linear gates remain
    assert 4 * written >= len(progs), written  # (gf2_linear counts Random gates too: the materialised sums on their own)


def test_crafted_program_cases(monkeypatch):
    monkeypatch.delenv("RV_LAZY_K", raising=False)
    prog, wit, wc = lazy_corpus.crafted_program()
    assert len(prog) <= 100 and wc[1] <= 40
    k1, k3 = _both(prog, wc, monkeypatch)
    # one Random gate plus the materialised sums, counted by hand from the rule (lazy_corpus.crafted_program)
    assert k3.gf2_rows_written == lazy_corpus.CRAFTED_MATERIALISED
    assert k3.gf2_linear == 1 + lazy_corpus.CRAFTED_MATERIALISED
    assert k1.gf2_rows_written > k3.gf2_rows_written
    assert k3.gf2_asserts == 3 and k3.gf2_muls == k1.gf2_muls
    # operand rows: the G_XORK gates' own plus what Mul and AssertZero gates read through their (up to three-row) forms
    assert k3.gf2_operand_rows > lazy_corpus.CRAFTED_XORK_ROWS


def test_getter_declared_and_exported():
    from reverie_amd import _lib

    header = open(os.path.join(ROOT, "include", "reverie_amd.h")).read()
    assert re.search(r"\bint\s+rv_circuit_compiled_on_device\s*\(\s*const\s+rv_circuit\s*\*\s*c\s*,\s*int\s*\*\s*on_device\s*\)\s*;", header)
    assert "rv_circuit_compiled_on_device" in _lib.SYMBOLS
    assert hasattr(_lib.lib(), "rv_circuit_compiled_on_device")
    assert _lib.lib().rv_abi_version() == 8
