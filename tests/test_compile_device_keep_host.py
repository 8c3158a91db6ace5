"""RV_COMPILE_DEVICE_KEEP_WIRES without a GPU: the header, the ctypes binding and the Python keywords agree on the bit, and the
argument checks that run before any device is touched."""
import ctypes as C
import os
import re

import pytest

from reverie_amd import _lib
from reverie_amd.ops import GF2, Z64, program

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RV_E_ARG = 9
WP, KEEP, DEV, Z, B, DK = 1, 2, 4, 8, 32, 128
SETTERS = ("rv_ctx_set_compile_flags", "rv_stream_set_compile_flags", "rv_eval_stream_set_compile_flags")


def header():
    return open(os.path.join(ROOT, "include", "reverie_amd.h")).read()


def _compile_ex(flags, prog=None):
    L = _lib.lib()
    h = C.c_void_p()
    if prog is None:
        return L.rv_circuit_compile_ex(None, None, C.c_size_t(0), C.c_size_t(1), C.c_size_t(4), C.c_uint32(flags), C.byref(h))
    return L.rv_circuit_compile_ex(None, prog.ctypes.data_as(C.c_void_p), C.c_size_t(len(prog)), C.c_size_t(1), C.c_size_t(4), C.c_uint32(flags),
                                   C.byref(h))


def test_bit_value_agrees():
    m = re.search(r"^#define RV_COMPILE_DEVICE_KEEP_WIRES (\d+)u", header(), re.M)
    assert m and int(m.group(1)) == 128 == _lib.RV_COMPILE_DEVICE_KEEP_WIRES
    others = [_lib.RV_COMPILE_WHOLE_PROVER, _lib.RV_COMPILE_KEEP_WIRES, _lib.RV_COMPILE_DEVICE, _lib.RV_COMPILE_DEVICE_Z64, _lib.RV_COMPILE_DEVICE_B2A]
    assert others == [1, 2, 4, 8, 32]
    for o in others:
        assert o & _lib.RV_COMPILE_DEVICE_KEEP_WIRES == 0
        assert int(re.search(r"^#define %s (\d+)u" % {1: "RV_COMPILE_WHOLE_PROVER", 2: "RV_COMPILE_KEEP_WIRES", 4: "RV_COMPILE_DEVICE",
                                                      8: "RV_COMPILE_DEVICE_Z64", 32: "RV_COMPILE_DEVICE_B2A"}[o], header(), re.M).group(1)) == o


def test_abi_version_stays():
    assert _lib.lib().rv_abi_version() == 8


def test_bit_without_its_partners_is_refused_before_the_device():
    L = _lib.lib()
    prog = program([GF2.Input(0), GF2.Input(1), GF2.Add(2, 0, 1)])
    for flags, missing in ((DK, b"RV_COMPILE_DEVICE_KEEP_WIRES needs RV_COMPILE_KEEP_WIRES and RV_COMPILE_DEVICE"),
                           (DK | DEV, b"RV_COMPILE_DEVICE_KEEP_WIRES needs RV_COMPILE_KEEP_WIRES"),
                           (DK | KEEP, b"RV_COMPILE_DEVICE_KEEP_WIRES needs RV_COMPILE_DEVICE")):
        for extra in (0, WP):
            for p in (None, prog):
                assert _compile_ex(flags | extra, p) == RV_E_ARG
                err = L.rv_last_error()
                assert b"rv_circuit_compile_ex" in err and err.endswith(missing), (flags, err)
    # with both partners the flag check passes, in every combination with the other bits: what is refused then is the NULL context
    for extra in (0, WP, Z, Z | B, WP | Z | B):
        assert _compile_ex(DK | KEEP | DEV | extra, prog) == RV_E_ARG
        assert b"NULL context" in L.rv_last_error(), extra
    # the older bits' rules still hold beside the new bit
    assert _compile_ex(DK | KEEP | DEV | B, prog) == RV_E_ARG and L.rv_last_error().endswith(b"RV_COMPILE_DEVICE_B2A needs RV_COMPILE_DEVICE_Z64")
    # the hook and the device entry point refuse the bit without its partners too (rv_circuit_compile_device implies RV_COMPILE_DEVICE)
    path, diff, h = C.c_int(), C.c_int(), C.c_void_p()
    for flags in (DK, DK | DEV, DK | KEEP):
        assert L.rv_hook_compile_compare_device(None, None, 0, 1, 4, flags, C.byref(path), C.byref(diff)) == RV_E_ARG
    for flags in (DK, DK | DEV):
        assert L.rv_circuit_compile_device(None, None, C.c_size_t(0), C.c_size_t(1), C.c_size_t(4), C.c_uint32(flags), C.byref(h)) == RV_E_ARG


def test_whole_programs_only():
    """the contexts' and the streams' flags are the three device bits: a stream's pieces write their wires back"""
    L = _lib.lib()
    start = (C.c_uint64 * 6)()
    path, diff = C.c_int(), C.c_int()
    for flags in (DK | DEV, DK, DK | DEV | Z | B, DK | KEEP | DEV):
        for name in SETTERS:
            assert getattr(L, name)(None, C.c_uint32(flags)) == RV_E_ARG
            err = L.rv_last_error()
            assert name.encode() in err and b"unknown flag bits" in err, (name, flags, err)
        assert L.rv_hook_compile_compare_device_chunk_ex(None, None, 0, 1, 4, start, flags, C.byref(path), C.byref(diff)) == RV_E_ARG


def test_bits_16_and_64_stay_unknown():
    L = _lib.lib()
    for flags in (16 | DK, 64 | DK, 16 | DK | KEEP | DEV, 64 | DK | KEEP | DEV, 16 | 64 | DK | KEEP | DEV | Z | B, 256 | DK | KEEP | DEV):
        assert _compile_ex(flags) == RV_E_ARG and b"unknown flag bits" in L.rv_last_error(), flags
        for name in SETTERS:
            assert getattr(L, name)(None, C.c_uint32(flags)) == RV_E_ARG and b"unknown flag bits" in L.rv_last_error(), (name, flags)


def test_keyword_needs_its_partners():
    import reverie_amd

    prog = program([Z64.Input(0)])
    with pytest.raises(ValueError, match=r"device_keep_wires=True needs keep_wires=True and device_compile=True"):
        reverie_amd.Circuit(prog, (1, 0), device_keep_wires=True)
    with pytest.raises(ValueError, match=r"device_keep_wires=True needs keep_wires=True$"):
        reverie_amd.Circuit(prog, (1, 0), device_keep_wires=True, device_compile=True)
    with pytest.raises(ValueError, match=r"device_keep_wires=True needs device_compile=True$"):
        reverie_amd.Circuit(prog, (1, 0), device_keep_wires=True, keep_wires=True)
    # from_device_ops is the device compile itself: keep_wires is what can be missing (checked before the tensor is looked at)
    with pytest.raises(ValueError, match=r"device_keep_wires=True needs keep_wires=True$"):
        reverie_amd.Circuit.from_device_ops(None, (1, 0), device_keep_wires=True)
    with pytest.raises(ValueError, match="device_b2a"):  # (the older checks stand beside the new keyword)
        reverie_amd.Circuit(prog, (1, 0), keep_wires=True, device_compile=True, device_keep_wires=True, device_b2a=True)


def test_cli_hands_the_compiler_to_the_gpu_evaluator(monkeypatch, tmp_path):
    """argument plumbing only: evaluate_gpu is replaced, nothing touches a GPU"""
    from reverie_amd import __main__ as cli

    seen = []
    monkeypatch.setattr(cli, "evaluate_gpu", lambda prog, wc, wit, compiler="host": seen.append(compiler))
    wit = tmp_path / "w.txt"
    wit.write_text("10")
    path = tmp_path / "p.rvops"
    program([GF2.Input(0), GF2.Input(1), GF2.Add(2, 0, 1)]).tofile(path)
    for compiler in ("host", "device", "device-z64", "device-b2a"):
        assert cli.main(["--operation", "oneshot", "--evaluator", "gpu", "--compiler", compiler, "--program-path", str(path),
                         "--witness-path", str(wit)]) == 0
    assert seen == ["host", "device", "device-z64", "device-b2a"]


def test_gpu_evaluator_compiles_with_the_new_bit(monkeypatch):
    """evaluate_gpu -> Circuit: the class is replaced, nothing touches a GPU"""
    from reverie_amd import __main__ as cli
    from reverie_amd import proof

    seen = []

    class Stop(Exception):
        pass

    def fake(prog, wc, **kw):
        seen.append(kw)
        raise Stop

    monkeypatch.setattr(proof, "Circuit", fake)
    for compiler in ("host", "device", "device-z64", "device-b2a"):
        with pytest.raises(Stop):
            cli.evaluate_gpu(program([GF2.Input(0)]), (0, 1), [1], compiler)
    base = {"keep_wires": True, "device_compile": True, "device_keep_wires": True}
    assert seen == [{}, dict(base, device_z64=False, device_b2a=False), dict(base, device_z64=True, device_b2a=False),
                    dict(base, device_z64=True, device_b2a=True)]
