"""rv_prove_batch_device / rv_verify_batch_device without a GPU: the header declares the entry points, the built library exports
them with the argument types the binding declares, and the Python functions refuse what is not a proof in GPU memory before any
library call (no context is made: there is no GPU here to make one on)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from conftest import ROOT

NEW = ("rv_prove_batch_device", "rv_verify_batch_device", "rv_hook_verify_batch_device_paths")


@pytest.fixture(scope="module")
def L():
    from reverie_amd import _lib

    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__

        __graft_entry__.build()
    return _lib.lib()


def test_header_declares_the_entry_points():
    hdr = open(os.path.join(ROOT, "include", "reverie_amd.h")).read()
    for name in NEW:
        assert re.search(r"\bint\s+" + name + r"\s*\(", hdr), name
    # the documented proof length, the destination's rules and the verifier's definition
    assert "32 + 4*8 + 40 * (gf2 + z64 online record sizes" in hdr
    assert re.search(r"rv_prove_batch_device\(rv_ctx \*ctx, const rv_circuit \*c, size_t batch,[^;]*void \*dst_device, size_t stride, size_t \*proof_len\);", hdr)
    assert re.search(r"rv_verify_batch_device\(rv_ctx \*ctx, const rv_circuit \*c, size_t batch, const uint8_t \*const \*d_proofs[^;]*"
                     r"const size_t \*proof_lens, uint32_t flags, int \*ok[^;]*\);", hdr)


def test_library_exports_them(L):
    import reverie_amd
    from reverie_amd import _lib

    for name in NEW:
        assert name in _lib.SYMBOLS and name in _lib.ARGTYPES
        fn = getattr(L, name)
        assert fn.argtypes is not None and fn.restype is C.c_int
    assert L.rv_abi_version() == 8  # (additive exports do not move it)
    assert reverie_amd.prove_batch_device is reverie_amd.proof.prove_batch_device
    assert reverie_amd.verify_batch_device is reverie_amd.proof.verify_batch_device
    out = (C.c_uint64 * 3)()
    assert L.rv_hook_verify_batch_device_paths(out) == 0 and L.rv_hook_verify_batch_device_paths(None) == 9
    # null arguments are refused before a device is touched
    ok = (C.c_int * 1)()
    n = C.c_size_t()
    assert L.rv_verify_batch_device(None, None, 1, None, None, 0, ok) == 9
    assert L.rv_prove_batch_device(None, None, 1, None, 0, None, 0, None, None, 256, C.byref(n)) == 9


def test_python_refuses_what_is_not_in_gpu_memory(monkeypatch):
    import torch

    import reverie_amd

    def no_context(*a, **k):
        raise AssertionError("a context was made")

    monkeypatch.setattr(reverie_amd.Context, "default", classmethod(no_context))
    monkeypatch.setattr(reverie_amd.Context, "__init__", no_context)
    sections = reverie_amd.DeviceProof.__new__(reverie_amd.DeviceProof)  # (a sections-form proof, without the GPU tensor it would hold)
    sections.lens, sections._comm, sections._ptr, sections.ctx, sections.tensor = [16, 16, 16, 16], bytes(32), 0, None, None
    for what in (torch.zeros(64, dtype=torch.uint8), sections, bytes(64), np.zeros(64, np.uint8), None):
        with pytest.raises(TypeError):
            reverie_amd.verify_batch_device(None, [what])
    with pytest.raises(TypeError):
        reverie_amd.prove_batch_device([], np.zeros((2, 4), np.uint8))
    assert reverie_amd.verify_batch_device.__doc__ and reverie_amd.prove_batch_device.__doc__
