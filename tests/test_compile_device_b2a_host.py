"""RV_COMPILE_DEVICE_B2A without a GPU: the header, the ctypes binding and the Python keywords agree on the bit, and the argument
checks that run before any device is touched."""
import ctypes as C
import os
import re

import pytest

from reverie_amd import _lib
from reverie_amd.ops import B2A, GF2, Z64, program

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RV_E_ARG = 9
WP, KEEP, DEV, Z, B = 1, 2, 4, 8, 32


def header():
    return open(os.path.join(ROOT, "include", "reverie_amd.h")).read()


def test_bit_value_agrees():
    m = re.search(r"^#define RV_COMPILE_DEVICE_B2A (\d+)u", header(), re.M)
    assert m and int(m.group(1)) == 32 == _lib.RV_COMPILE_DEVICE_B2A
    others = _lib.RV_COMPILE_WHOLE_PROVER | _lib.RV_COMPILE_KEEP_WIRES | _lib.RV_COMPILE_DEVICE | _lib.RV_COMPILE_DEVICE_Z64
    assert others == 15 and _lib.RV_COMPILE_DEVICE_B2A & others == 0
    # the header says why 16 is skipped
    assert re.search(r"RV_COMPILE_DEVICE_B2A.*?\b16\b.*?unknown", header(), re.S)
    assert _lib.lib().rv_abi_version() == 8


def _compile_ex(flags, prog=None):
    L = _lib.lib()
    h = C.c_void_p()
    if prog is None:
        return L.rv_circuit_compile_ex(None, None, C.c_size_t(0), C.c_size_t(1), C.c_size_t(64), C.c_uint32(flags), C.byref(h))
    return L.rv_circuit_compile_ex(None, prog.ctypes.data_as(C.c_void_p), C.c_size_t(len(prog)), C.c_size_t(1), C.c_size_t(64), C.c_uint32(flags),
                                   C.byref(h))


def test_bit_without_both_others_is_refused_before_the_device():
    L = _lib.lib()
    prog = program([GF2.Input(i) for i in range(64)] + [B2A(0, 0), Z64.AddConst(0, 0, 5)])
    # what is missing is named: the Z64 bit, the device bit, or both
    for flags, missing in ((B, b"RV_COMPILE_DEVICE_B2A needs RV_COMPILE_DEVICE and RV_COMPILE_DEVICE_Z64"),
                           (B | DEV, b"RV_COMPILE_DEVICE_B2A needs RV_COMPILE_DEVICE_Z64"),
                           (B | Z, b"RV_COMPILE_DEVICE_B2A needs RV_COMPILE_DEVICE")):
        for extra in (0, WP, KEEP):
            assert _compile_ex(flags | extra, prog) == RV_E_ARG
            err = L.rv_last_error()
            assert b"rv_circuit_compile_ex" in err and err.endswith(missing), (flags, err)
        for name in ("rv_ctx_set_compile_flags", "rv_stream_set_compile_flags", "rv_eval_stream_set_compile_flags"):
            assert getattr(L, name)(None, C.c_uint32(flags)) == RV_E_ARG
            err = L.rv_last_error()
            assert name.encode() in err and err.endswith(missing), (name, flags, err)
    # all three bits pass the flag check: what is refused then is the NULL handle
    assert _compile_ex(DEV | Z | B, prog) == RV_E_ARG and b"NULL context" in L.rv_last_error()
    for name in ("rv_ctx_set_compile_flags", "rv_stream_set_compile_flags", "rv_eval_stream_set_compile_flags"):
        assert getattr(L, name)(None, C.c_uint32(DEV | Z | B)) == RV_E_ARG
    # the hooks and the device entry point refuse the lone bit too (a NULL context is an argument error of its own)
    path, diff, h = C.c_int(), C.c_int(), C.c_void_p()
    start = (C.c_uint64 * 6)()
    assert L.rv_hook_compile_compare_device(None, None, 0, 1, 64, B | DEV, C.byref(path), C.byref(diff)) == RV_E_ARG
    assert L.rv_hook_compile_compare_device_chunk_ex(None, None, 0, 1, 64, start, B | DEV, C.byref(path), C.byref(diff)) == RV_E_ARG
    assert L.rv_circuit_compile_device(None, None, C.c_size_t(0), C.c_size_t(1), C.c_size_t(64), C.c_uint32(B), C.byref(h)) == RV_E_ARG


def test_flag_16_is_still_unknown():
    L = _lib.lib()
    for flags in (16, 16 | DEV | Z | B, 64, 1 << 31):
        assert _compile_ex(flags) == RV_E_ARG and b"unknown flag bits" in L.rv_last_error(), flags
    for name in ("rv_ctx_set_compile_flags", "rv_stream_set_compile_flags", "rv_eval_stream_set_compile_flags"):
        assert getattr(L, name)(None, C.c_uint32(16 | DEV | Z)) == RV_E_ARG and b"unknown flag bits" in L.rv_last_error()
        # (the context's and the streams' flags are the three device bits only)
        assert getattr(L, name)(None, C.c_uint32(WP | DEV | Z | B)) == RV_E_ARG and b"unknown flag bits" in L.rv_last_error()


def test_keyword_needs_both_other_keywords():
    import reverie_amd
    from reverie_amd import stream

    prog = program([Z64.Input(0)])
    for kw in ({}, {"device_compile": True}):
        with pytest.raises(ValueError, match="device_b2a"):
            reverie_amd.Circuit(prog, (1, 0), device_b2a=True, **kw)
    with pytest.raises(ValueError):  # (device_z64 without device_compile: the older check)
        reverie_amd.Circuit(prog, (1, 0), device_b2a=True, device_z64=True)
    for cls, args in ((stream.StreamingProver, ((1, 0),)), (stream.StreamingVerifier, ((1, 0), b"")), (stream.StreamingBatchProver, ((1, 0), 2)),
                      (stream.StreamingBatchVerifier, ((1, 0), [b""])), (stream.StreamingEvaluator, ((1, 0),))):
        for kw in ({}, {"device_compile": True}):
            with pytest.raises(ValueError, match="device_b2a"):
                cls(*args, device_b2a=True, **kw)
    for f, args in ((stream.prove_streaming, (prog, [], [1], (1, 0))), (stream.verify_streaming, (prog, (1, 0), b"")),
                    (stream.prove_streaming_batch, (prog, [], [[1]], (1, 0))), (stream.verify_streaming_batch, (prog, (1, 0), [b""])),
                    (stream.evaluate_streaming, (prog, [], [1], (1, 0)))):
        for kw in ({}, {"device_compile": True}):
            with pytest.raises(ValueError, match="device_b2a"):
                f(*args, device_b2a=True, **kw)
    assert stream._device_flags(True, True, True) == 44
    assert stream._device_flags(True, True) == 12 and stream._device_flags(True, False) == 4 and stream._device_flags(False, False) == 0
    for dc, dz in ((False, False), (True, False), (False, True)):
        with pytest.raises(ValueError):
            stream._device_flags(dc, dz, True)


def test_cli_choice():
    from reverie_amd.__main__ import build_parser

    ap = build_parser()
    for choice in ("host", "device", "device-z64", "device-b2a"):
        assert ap.parse_args(["--operation", "version_info", "--compiler", choice]).compiler == choice


def test_cli_passes_device_b2a_to_the_streaming_evaluator(monkeypatch, tmp_path):
    """argument plumbing only: evaluate_stream is replaced, nothing touches a GPU"""
    from reverie_amd import __main__ as cli

    seen = {}
    monkeypatch.setattr(cli, "evaluate_stream", lambda *a, **kw: seen.update(kw))
    wit = tmp_path / "w.txt"
    wit.write_text("101")
    for compiler, want in (("device-b2a", {"device_compile": True, "device_z64": True, "device_b2a": True}),
                           ("device-z64", {"device_compile": True, "device_z64": True}), ("device", {"device_compile": True}),
                           ("host", {"device_compile": False})):
        seen.clear()
        assert cli.main(["--operation", "oneshot", "--evaluator", "stream", "--compiler", compiler, "--program-path", "p.rvops", "--witness-path", str(wit)]) == 0
        assert seen == want, compiler


def test_evaluate_stream_hands_the_keyword_on(monkeypatch, tmp_path):
    """evaluate_stream -> StreamingEvaluator: the class is replaced, nothing touches a GPU"""
    import numpy as np

    from reverie_amd import __main__ as cli
    from reverie_amd import stream
    from reverie_amd.ops import OP_DTYPE

    seen = {}

    class Stop(Exception):
        pass

    def fake(*a, **kw):
        seen.update(kw)
        raise Stop

    monkeypatch.setattr(stream, "StreamingEvaluator", fake)
    path = tmp_path / "p.rvops"
    np.zeros(0, OP_DTYPE).tofile(path)
    with pytest.raises(Stop):
        cli.evaluate_stream(str(path), "rvops", None, [1], 0, device_compile=True, device_z64=True, device_b2a=True)
    assert seen == {"device_compile": True, "device_z64": True, "device_b2a": True}
