"""RV_COMPILE_DEVICE_Z64 without a GPU: the header, the ctypes binding and the Python keywords agree on the bit, and the argument
checks that run before any device is touched."""
import ctypes as C
import os
import re

import pytest

from reverie_amd import _lib
from reverie_amd.ops import GF2, Z64, program

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RV_E_ARG = 9


def header():
    return open(os.path.join(ROOT, "include", "reverie_amd.h")).read()


def test_bit_value_agrees():
    m = re.search(r"^#define RV_COMPILE_DEVICE_Z64 (\d+)u", header(), re.M)
    assert m and int(m.group(1)) == 8 == _lib.RV_COMPILE_DEVICE_Z64
    m = re.search(r"^#define RV_COMPILE_DEVICE (\d+)u", header(), re.M)
    assert m and int(m.group(1)) == 4 == _lib.RV_COMPILE_DEVICE
    # one bit of its own beside the three older flags
    assert _lib.RV_COMPILE_DEVICE_Z64 & (_lib.RV_COMPILE_WHOLE_PROVER | _lib.RV_COMPILE_KEEP_WIRES | _lib.RV_COMPILE_DEVICE) == 0
    for sym in ("rv_hook_compile_compare_device_chunk_ex", "rv_hook_compile_device_laps_z64"):
        assert sym in _lib.SYMBOLS and re.search(r"\b%s\(" % sym, header())
    assert _lib.lib().rv_abi_version() == 8


def test_bit_alone_is_refused_before_the_device():
    L = _lib.lib()
    prog = program([Z64.Input(0), GF2.Input(0)])
    h = C.c_void_p()
    for flags in (8, 8 | 1, 8 | 2):
        rc = L.rv_circuit_compile_ex(None, prog.ctypes.data_as(C.c_void_p), C.c_size_t(len(prog)), C.c_size_t(1), C.c_size_t(1), C.c_uint32(flags),
                                     C.byref(h))
        assert rc == RV_E_ARG and b"RV_COMPILE_DEVICE_Z64 needs RV_COMPILE_DEVICE" in L.rv_last_error()
    rc = L.rv_circuit_compile_ex(None, None, C.c_size_t(0), C.c_size_t(1), C.c_size_t(1), C.c_uint32(16), C.byref(h))
    assert rc == RV_E_ARG and b"unknown flag bits" in L.rv_last_error()
    path, diff = C.c_int(), C.c_int()
    start = (C.c_uint64 * 6)()
    # (a NULL context is an argument error of its own: these only show that the calls exist and refuse)
    assert L.rv_hook_compile_compare_device_chunk_ex(None, None, 0, 1, 1, start, 8, C.byref(path), C.byref(diff)) == RV_E_ARG
    assert L.rv_ctx_set_compile_flags(None, 8) == RV_E_ARG
    assert L.rv_stream_set_compile_flags(None, 12) == RV_E_ARG
    assert L.rv_eval_stream_set_compile_flags(None, 12) == RV_E_ARG


def test_keyword_needs_device_compile():
    import reverie_amd
    from reverie_amd import stream

    prog = program([Z64.Input(0)])
    with pytest.raises(ValueError):
        reverie_amd.Circuit(prog, (1, 0), device_z64=True)
    for cls, args in ((stream.StreamingProver, ((1, 0),)), (stream.StreamingVerifier, ((1, 0), b"")), (stream.StreamingBatchProver, ((1, 0), 2)),
                      (stream.StreamingBatchVerifier, ((1, 0), [b""])), (stream.StreamingEvaluator, ((1, 0),))):
        with pytest.raises(ValueError, match="device_z64"):
            cls(*args, device_z64=True)
    for f, args in ((stream.prove_streaming, (prog, [], [1], (1, 0))), (stream.verify_streaming, (prog, (1, 0), b"")),
                    (stream.prove_streaming_batch, (prog, [], [[1]], (1, 0))), (stream.verify_streaming_batch, (prog, (1, 0), [b""])),
                    (stream.evaluate_streaming, (prog, [], [1], (1, 0)))):
        with pytest.raises(ValueError, match="device_z64"):
            f(*args, device_z64=True)
    assert stream._device_flags(True, True) == 12 and stream._device_flags(True, False) == 4 and stream._device_flags(False, False) == 0


def test_cli_choice():
    from reverie_amd.__main__ import build_parser

    ap = build_parser()
    for choice in ("host", "device", "device-z64"):
        assert ap.parse_args(["--operation", "version_info", "--compiler", choice]).compiler == choice


def test_cli_passes_device_z64_to_the_streaming_evaluator(monkeypatch, tmp_path):
    """argument plumbing only: evaluate_stream is replaced, nothing touches a GPU"""
    from reverie_amd import __main__ as cli

    seen = {}
    monkeypatch.setattr(cli, "evaluate_stream", lambda *a, **kw: seen.update(kw))
    wit = tmp_path / "w.txt"
    wit.write_text("101")
    for compiler, want in (("device-z64", {"device_compile": True, "device_z64": True}), ("device", {"device_compile": True}), ("host", {"device_compile": False})):
        seen.clear()
        assert cli.main(["--operation", "oneshot", "--evaluator", "stream", "--compiler", compiler, "--program-path", "p.rvops", "--witness-path", str(wit)]) == 0
        assert seen == want, compiler
