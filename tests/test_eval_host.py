"""Cleartext evaluation, host side (no GPU): the C-ABI additions, the compilers' wire tables, the CLI switch."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from reverie_amd.ops import GF2, OP_DTYPE, Z64, program

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = open(os.path.join(ROOT, "include", "reverie_amd.h")).read()
NEW = ("rv_evaluate", "rv_evaluate_batch", "rv_hook_eval_schedules")


@pytest.fixture(scope="module")
def L():
    from reverie_amd import _lib

    return _lib.lib()


def test_new_symbols_exported_and_typed(L):
    from reverie_amd import _lib

    declared = set(re.findall(r"\b(rv_[a-z0-9_]+)\s*\(", HDR))
    for name in NEW:
        assert name in declared and name in _lib.SYMBOLS
        assert getattr(L, name).restype is C.c_int
    assert int(re.search(r"#define RV_COMPILE_KEEP_WIRES (\d+)u", HDR).group(1)) == _lib.RV_COMPILE_KEEP_WIRES == 2
    body = re.search(r"typedef struct rv_eval_status \{(.*?)\} rv_eval_status;", HDR, re.S).group(1)
    fields = re.findall(r"uint64_t (\w+);", body)
    assert fields == [n for n, _ in _lib.EvalStatus._fields_] == ["n_failed", "first_failed_op"]
    assert C.sizeof(_lib.EvalStatus) == 16 and _lib.EvalStatus.first_failed_op.offset == 8


def test_compile_ex_accepts_keep_wires_only_as_a_new_flag(L):
    # no device needed to see the argument check: an unknown flag is refused before the context is looked at
    h = C.c_void_p()
    assert L.rv_circuit_compile_ex(None, None, 0, 0, 0, C.c_uint32(4), C.byref(h)) == 9


def _random_gf2(rng, n_ops, n_wires=20000, n_z64=400, p_z64=0.15):
    """a long program (parallel compiler) over recycled wires: every GF(2) opcode but Random, Z64 gates, wires never written"""
    ops = [GF2.Input(w) for w in range(64)] + [Z64.Input(w) for w in range(8)]
    kinds = rng.choice(8, n_ops, p=[0.03, 0.25, 0.08, 0.12, 0.28, 0.06, 0.06, 0.12])
    d = rng.integers(0, n_wires - 20, n_ops)  # (the last 20 wires are never written)
    a = rng.integers(0, n_wires, n_ops)
    b = rng.integers(0, n_wires, n_ops)
    z = rng.random(n_ops) < p_z64
    for i in range(n_ops):
        k, di, ai, bi = int(kinds[i]), int(d[i]), int(a[i]), int(b[i])
        if z[i]:
            di, ai, bi = di % n_z64, ai % n_z64, bi % n_z64
            ops.append([Z64.Input(di), Z64.Add(di, ai, bi), Z64.AddConst(di, ai, 5), Z64.Sub(di, ai, bi), Z64.Mul(di, ai, bi),
                        Z64.MulConst(di, ai, 3), Z64.AssertZero(ai), Z64.Const(di, 7)][k])
        else:
            ops.append([GF2.Input(di), GF2.Add(di, ai, bi), GF2.AddConst(di, ai, 1), GF2.Sub(di, ai, bi), GF2.Mul(di, ai, bi),
                        GF2.MulConst(di, ai, 1), GF2.AssertZero(ai), GF2.Const(di, 1)][k])
    return program(ops), (n_z64, n_wires)


def _compare(L, prog, wc, flags, threads=4):
    d = C.c_int(-7)
    rc = L.rv_hook_compile_compare(prog.ctypes.data_as(C.c_void_p), C.c_size_t(len(prog)), C.c_size_t(wc[0]), C.c_size_t(wc[1]),
                                   C.c_uint32(flags), C.c_int(threads), C.byref(d))
    return rc, d.value


@pytest.mark.parametrize("seed", [1, 2])
def test_parallel_compiler_keeps_the_same_wire_tables(L, seed):
    from reverie_amd import _lib

    prog, wc = _random_gf2(np.random.default_rng(seed), 230_000)
    assert len(prog) > 200_000  # RV_COMPILE_PAR_MIN: what rv_circuit_compile_ex hands to the parallel compiler
    for flags in (_lib.RV_COMPILE_KEEP_WIRES, _lib.RV_COMPILE_KEEP_WIRES | _lib.RV_COMPILE_WHOLE_PROVER):
        for threads in (2, 5):
            assert _compare(L, prog, wc, flags, threads) == (0, 0), (flags, threads)


def _rvops(tmp_path, prog, name="p.rvops"):
    p = tmp_path / name
    p.write_bytes(np.ascontiguousarray(prog, OP_DTYPE).tobytes())
    return p


def test_cli_evaluator_switch(tmp_path):
    from reverie_amd.__main__ import build_parser, main, use_gpu_evaluator

    assert build_parser().parse_args(["--operation", "oneshot", "--evaluator", "gpu"]).evaluator == "gpu"
    assert build_parser().parse_args(["--operation", "oneshot"]).evaluator == "auto"
    with pytest.raises(SystemExit):
        build_parser().parse_args(["--operation", "oneshot", "--evaluator", "cpu"])
    small2 = program([GF2.Input(0), GF2.AddConst(1, 0, 1)])
    mixed = program([GF2.Input(0), Z64.Const(0, 3)])
    assert not use_gpu_evaluator(small2, "auto") and use_gpu_evaluator(mixed, "auto") and use_gpu_evaluator(small2, "gpu")
    assert not use_gpu_evaluator(mixed, "host")
    # the host evaluator keeps its message for programs it cannot run
    w = tmp_path / "w.txt"
    w.write_text("1\n")
    with pytest.raises(SystemExit) as e:
        main(["--operation", "oneshot", "--evaluator", "host", "--program-path", str(_rvops(tmp_path, mixed)), "--witness-path", str(w)])
    assert "oneshot supports GF(2) programs only" in str(e.value)
