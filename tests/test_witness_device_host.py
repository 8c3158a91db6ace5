"""The witness-from-device-memory entry points (rv_prove_wdev, rv_prove_device_wdev, rv_prove_batch_wdev,
rv_prove_batch_device_wdev, rv_evaluate_batch_device, rv_hook_witness_traffic) without a GPU: the header declares them and the
descriptor, the built library exports them with the argument types the binding declares, NULL arguments are refused before a
device is touched, and the Python functions refuse witnesses that are half on the host before any context is made."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from conftest import ROOT

NEW = ("rv_prove_wdev", "rv_prove_device_wdev", "rv_prove_batch_wdev", "rv_prove_batch_device_wdev", "rv_evaluate_batch_device",
       "rv_hook_witness_traffic")
E_ARG = 9


@pytest.fixture(scope="module")
def L():
    from reverie_amd import _lib

    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__

        __graft_entry__.build()
    return _lib.lib()


def test_header_declares_the_entry_points_and_the_struct():
    hdr = open(os.path.join(ROOT, "include", "reverie_amd.h")).read()
    for name in NEW:
        assert re.search(r"\bint\s+" + name + r"\s*\(", hdr), name
    m = re.search(r"typedef struct rv_dev_witness \{(.*?)\} rv_dev_witness;", hdr, re.S)
    assert m
    fields = re.findall(r"(const uint8_t \*|const uint64_t \*|size_t )(\w+);", m.group(1))
    assert fields == [("const uint8_t *", "gf2"), ("size_t ", "n_gf2"), ("size_t ", "stride_gf2"),
                      ("const uint64_t *", "z64"), ("size_t ", "n_z64"), ("size_t ", "stride_z64")]
    assert re.search(r"rv_prove_wdev\(rv_ctx \*ctx, const rv_circuit \*c, const rv_dev_witness \*w, const uint8_t \*seeds, uint8_t \*\*proof, "
                     r"size_t \*proof_len\);", hdr)
    assert re.search(r"rv_evaluate_batch_device\(rv_ctx \*ctx, const rv_circuit \*c, size_t batch, const rv_dev_witness \*w, const uint32_t \*sel_gf2,"
                     r"[^;]*uint8_t \*d_gf2_values, uint64_t \*d_z64_values,\s*rv_eval_status \*d_status\);", hdr)
    assert re.search(r"rv_hook_witness_traffic\(uint64_t out\[3\]\);", hdr)
    # the streams' header comment no longer reads as if no call took witnesses from device memory
    assert "The witnesses stay in host memory" not in hdr and "streams still take their witnesses from host memory" in hdr


def test_library_exports_them(L):
    import reverie_amd
    from reverie_amd import _lib

    for name in NEW:
        assert name in _lib.SYMBOLS and name in _lib.ARGTYPES
        fn = getattr(L, name)
        assert fn.argtypes is not None and fn.restype is C.c_int
    for name in NEW[:5]:
        assert C.POINTER(_lib.DevWitness) in _lib.ARGTYPES[name]
    assert C.sizeof(_lib.DevWitness) == 48
    assert [f[0] for f in _lib.DevWitness._fields_] == ["gf2", "n_gf2", "stride_gf2", "z64", "n_z64", "stride_z64"]
    assert L.rv_abi_version() == 8  # (additive exports do not move it)
    assert reverie_amd.DeviceEvaluation is reverie_amd.proof.DeviceEvaluation
    assert reverie_amd.Circuit.evaluate_batch_device.__doc__ and reverie_amd.proof._device_witness.__doc__
    out = (C.c_uint64 * 3)()
    assert L.rv_hook_witness_traffic(out) == 0 and L.rv_hook_witness_traffic(None) == E_ARG


def test_null_arguments_are_refused_before_a_device_is_touched(L):
    from reverie_amd import _lib

    w = _lib.DevWitness()
    fake = C.c_void_p(8)  # (never dereferenced: every call below has a NULL among the three it checks first)
    proof, n = C.c_void_p(), C.c_size_t()
    proofs, lens = (C.c_void_p * 2)(), (C.c_size_t * 2)()
    comm, omit, lens4 = (C.c_uint8 * 32)(), (C.c_uint8 * 256)(), (C.c_size_t * 4)()
    seeds = (C.c_uint8 * (2 * 256 * 16))()
    st = (C.c_uint64 * 4)()
    before = (C.c_uint64 * 3)()
    assert L.rv_hook_witness_traffic(before) == 0
    for ctx, c, dw in ((None, fake, C.byref(w)), (fake, None, C.byref(w)), (fake, fake, None), (None, None, None)):
        assert L.rv_prove_wdev(ctx, c, dw, seeds, C.byref(proof), C.byref(n)) == E_ARG
        assert L.rv_prove_device_wdev(ctx, c, dw, seeds, fake, comm, omit, lens4) == E_ARG
        assert L.rv_prove_batch_wdev(ctx, c, 2, dw, seeds, proofs, lens) == E_ARG
        assert L.rv_prove_batch_device_wdev(ctx, c, 2, dw, seeds, fake, 256, C.byref(n)) == E_ARG
        assert L.rv_evaluate_batch_device(ctx, c, 2, dw, None, 0, None, 0, None, None, st) == E_ARG
    out = (C.c_uint64 * 3)()
    assert L.rv_hook_witness_traffic(out) == 0 and list(out) == list(before)


def as_gpu_tensor(t):
    """a tensor that says it lies in GPU memory (there is no GPU here: what is under test refuses before it looks at the data)"""
    import torch

    class SaysCuda(torch.Tensor):
        @property
        def device(self):
            return torch.device("cuda", 0)

    return torch.Tensor._make_subclass(SaysCuda, t)


def test_python_refuses_mixed_and_host_witnesses(monkeypatch):
    import torch

    import reverie_amd

    def no_context(*a, **k):
        raise AssertionError("a context was made")

    monkeypatch.setattr(reverie_amd.Context, "default", classmethod(no_context))
    monkeypatch.setattr(reverie_amd.Context, "__init__", no_context)
    circuit = reverie_amd.Circuit.__new__(reverie_amd.Circuit)  # (a compiled circuit, without the GPU it would live on)
    circuit.ctx, circuit.handle, circuit.wire_counts, circuit.keep_wires = None, C.c_void_p(), (2, 4), True
    g1, z1 = as_gpu_tensor(torch.zeros(4, dtype=torch.uint8)), as_gpu_tensor(torch.zeros(2, dtype=torch.int64))
    gB, zB = as_gpu_tensor(torch.zeros((3, 4), dtype=torch.uint8)), as_gpu_tensor(torch.zeros((3, 2), dtype=torch.int64))
    assert g1.device.type == "cuda" and isinstance(g1, torch.Tensor)
    for host_z in (np.ones(2, np.uint64), [1, 2], torch.ones(2, dtype=torch.int64)):
        with pytest.raises(TypeError):
            reverie_amd.Proof.new(circuit, g1, host_z)
        with pytest.raises(TypeError):
            reverie_amd.DeviceProof.new(circuit, g1, host_z)
    for host_g in (np.ones(4, np.uint8), [1, 0, 0, 1], torch.ones(4, dtype=torch.uint8)):
        with pytest.raises(TypeError):
            reverie_amd.Proof.new(circuit, host_g, z1)
        with pytest.raises(TypeError):
            reverie_amd.DeviceProof.new(circuit, host_g, z1)
    with pytest.raises(TypeError):
        reverie_amd.Proof.new_batch(circuit, gB, np.ones((3, 2), np.uint64))
    with pytest.raises(TypeError):
        reverie_amd.Proof.new_batch(circuit, np.ones((3, 4), np.uint8), zB)
    with pytest.raises(TypeError):
        reverie_amd.prove_batch_device(circuit, gB, np.ones((3, 2), np.uint64))
    with pytest.raises(TypeError):
        circuit.evaluate_batch_device(gB, np.ones((3, 2), np.uint64))
    # a CPU tensor, an array: evaluate_batch_device takes GPU memory only
    for what in (torch.zeros((3, 4), dtype=torch.uint8), np.zeros((3, 4), np.uint8), [[0, 1, 0, 1]]):
        with pytest.raises(TypeError):
            circuit.evaluate_batch_device(what)
    # a GPU tensor of a form the library does not read: refused as a value, still before any context
    for bad in (as_gpu_tensor(torch.zeros((3, 4), dtype=torch.float32)), as_gpu_tensor(torch.zeros((3, 8), dtype=torch.uint8)[:, ::2]), g1):
        with pytest.raises(ValueError):
            circuit.evaluate_batch_device(bad)
