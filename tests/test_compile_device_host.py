"""Host-side checks of the device compiler's interface (no GPU): the C-ABI additions are exported with the declared signatures,
rv_circuit_compile_ex knows RV_COMPILE_DEVICE and still refuses unknown flag bits and a NULL context, and the Python / CLI
surfaces exist and validate their arguments before any GPU work."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from conftest import ROOT

NEW = {
    "rv_circuit_compile_device": "int rv_circuit_compile_device(rv_ctx *ctx, const rv_op *d_ops, size_t n_ops, size_t z64_wires, size_t gf2_wires, "
                                 "uint32_t flags, rv_circuit **out)",
    "rv_ctx_set_compile_flags": "int rv_ctx_set_compile_flags(rv_ctx *ctx, uint32_t flags)",
    "rv_hook_compile_compare_device": "int rv_hook_compile_compare_device(rv_ctx *ctx, const rv_op *ops, size_t n_ops, size_t z64_wires, "
                                      "size_t gf2_wires, uint32_t flags, int *path, int *diff)",
    "rv_hook_compile_device_laps": "int rv_hook_compile_device_laps(double out[6])",
}


@pytest.fixture(scope="module")
def L():
    from reverie_amd import _lib

    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__

        __graft_entry__.build()
    return _lib.lib()


def _norm(s):
    return re.sub(r"\s+", " ", s.replace("( ", "(").replace(" )", ")")).strip()


def test_new_symbols_declared_and_exported(L):
    from reverie_amd import _lib

    hdr = _norm(re.sub(r"/\*.*?\*/", " ", open(os.path.join(ROOT, "include", "reverie_amd.h")).read(), flags=re.S))
    for name, sig in NEW.items():
        assert _norm(sig) + ";" in hdr, name
        assert name in _lib.SYMBOLS
        assert getattr(L, name) is not None
    assert re.search(r"#define RV_COMPILE_DEVICE 4u", open(os.path.join(ROOT, "include", "reverie_amd.h")).read())
    assert _lib.RV_COMPILE_DEVICE == 4
    assert L.rv_abi_version() == 8  # (pure additions)
    # ctypes signatures match the header's parameter counts
    for name, sig in NEW.items():
        n_params = sig[sig.index("(") + 1:sig.rindex(")")].count(",") + 1
        assert len(_lib.ARGTYPES[name]) == n_params, name


def _compile_ex(L, ctx, flags):
    from reverie_amd import _lib

    ops = np.zeros(1, dtype=[("x", np.uint8, 24)])
    out = C.c_void_p()
    return L.rv_circuit_compile_ex(ctx, ops.ctypes.data_as(C.c_void_p), C.c_size_t(1), C.c_size_t(0), C.c_size_t(1), C.c_uint32(flags),
                                   C.byref(out)), L.rv_last_error().decode()


def test_compile_ex_flags(L):
    from reverie_amd import _lib

    # an unknown bit is refused as such, before anything else is looked at
    for bad in (8, 16, 0x80000000, _lib.RV_COMPILE_DEVICE | 8):
        rc, err = _compile_ex(L, None, bad)
        assert rc == 9 and "flag" in err, (bad, rc, err)
    # RV_COMPILE_DEVICE (alone or with the other hints) passes the flag check: what is refused then is the NULL context
    for ok in (_lib.RV_COMPILE_DEVICE, _lib.RV_COMPILE_DEVICE | _lib.RV_COMPILE_WHOLE_PROVER, _lib.RV_COMPILE_DEVICE | _lib.RV_COMPILE_KEEP_WIRES):
        rc, err = _compile_ex(L, None, ok)
        assert rc == 9 and "NULL context" in err, (ok, rc, err)


def test_null_context_and_bad_arguments(L):
    from reverie_amd import _lib

    out = C.c_void_p()
    ops = np.zeros(4, np.uint8)
    assert L.rv_circuit_compile_device(None, ops.ctypes.data_as(C.c_void_p), 0, 0, 1, _lib.RV_COMPILE_DEVICE, C.byref(out)) == 9
    assert L.rv_ctx_set_compile_flags(None, 0) == 9
    assert L.rv_ctx_set_compile_flags(None, _lib.RV_COMPILE_DEVICE) == 9
    path, diff = C.c_int(-7), C.c_int(-7)
    assert L.rv_hook_compile_compare_device(None, ops.ctypes.data_as(C.c_void_p), 0, 0, 1, 0, C.byref(path), C.byref(diff)) == 9
    assert L.rv_hook_compile_device_laps(None) == 9
    laps = (C.c_double * 6)()
    assert L.rv_hook_compile_device_laps(laps) == 0


def test_python_surface():
    import inspect

    import reverie_amd

    assert "device_compile" in inspect.signature(reverie_amd.Circuit.__init__).parameters
    assert hasattr(reverie_amd.Circuit, "from_device_ops")
    assert hasattr(reverie_amd.Context, "set_compile_flags")
    # host memory is refused before any context or GPU is touched
    with pytest.raises(TypeError):
        reverie_amd.Circuit.from_device_ops(np.zeros((4, 24), np.uint8), (0, 4))
    torch = pytest.importorskip("torch")
    with pytest.raises(TypeError):
        reverie_amd.Circuit.from_device_ops(torch.zeros((4, 24), dtype=torch.uint8), (0, 4))


def test_cli_compiler_option():
    from reverie_amd.__main__ import build_parser

    ap = build_parser()
    a = ap.parse_args(["--operation", "prove", "--program-path", "p", "--witness-path", "w", "--proof-path", "o"])
    assert a.compiler == "host"
    a = ap.parse_args(["--operation", "verify", "--program-path", "p", "--proof-path", "o", "--compiler", "device"])
    assert a.compiler == "device"
    with pytest.raises(SystemExit):
        ap.parse_args(["--operation", "verify", "--compiler", "gpu"])
