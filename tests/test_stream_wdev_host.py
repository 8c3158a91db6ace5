"""Streams in device memory (witnesses in, proofs out, verification in place) -- what holds without a GPU: the seven entry points and
three hooks are declared in the header with their signatures, exported by the library and bound in _lib.py with matching argument
types, they are pure additions (the ABI version stays 8), NULL arguments are answered before any device is touched, and the Python
feeds refuse half-host witness pairs and CPU tensors before any context exists."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from reverie_amd import _lib

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "reverie_amd.h")
E_ARG = 9
NEW = {
    "rv_stream_feed_wdev": "int rv_stream_feed_wdev(rv_stream *s, const rv_op *ops, size_t n_ops, int ops_on_device, const rv_dev_witness *w);",
    "rv_eval_stream_feed_wdev": "int rv_eval_stream_feed_wdev(rv_eval_stream *s, const rv_op *ops, size_t n_ops, int ops_on_device, "
                                "const rv_dev_witness *w);",
    "rv_stream_finish_device": "int rv_stream_finish_device(rv_stream *s, void *dst_device, size_t cap, size_t *proof_len);",
    "rv_stream_finish_batch_device": "int rv_stream_finish_batch_device(rv_stream *s, void *dst_device, size_t stride, size_t *proof_len);",
    "rv_stream_verify_begin_device": "int rv_stream_verify_begin_device(rv_ctx *ctx, size_t z64_wires, size_t gf2_wires, const uint8_t *d_proof, "
                                     "size_t proof_len, size_t max_chunk_ops, rv_stream **out);",
    "rv_stream_verify_begin_batch_device": "int rv_stream_verify_begin_batch_device(rv_ctx *ctx, size_t z64_wires, size_t gf2_wires, size_t batch, "
                                           "const uint8_t *const *d_proofs /* host array of device pointers */, const size_t *proof_lens, "
                                           "size_t max_chunk_ops, rv_stream **out);",
    "rv_hook_stream_traffic": "int rv_hook_stream_traffic(uint64_t out[4]);",
    "rv_hook_stream_verify_device_paths": "int rv_hook_stream_verify_device_paths(uint64_t out[2]);",
    "rv_hook_stream_wit_sums": "int rv_hook_stream_wit_sums(rv_ctx *ctx, const uint8_t *gf2, size_t n_gf2, uint64_t first_gf2, const uint64_t *z64, "
                               "size_t n_z64, uint64_t first_z64, uint64_t *host_out, uint64_t *dev_out);",
}
N_ARGS = {"rv_stream_feed_wdev": 5, "rv_eval_stream_feed_wdev": 5, "rv_stream_finish_device": 4, "rv_stream_finish_batch_device": 4,
          "rv_stream_verify_begin_device": 7, "rv_stream_verify_begin_batch_device": 8, "rv_hook_stream_traffic": 1,
          "rv_hook_stream_verify_device_paths": 1, "rv_hook_stream_wit_sums": 9}


def test_declared_exported_and_bound():
    text = re.sub(r"\s+", " ", open(HEADER).read())
    L = _lib.lib()
    for name, decl in NEW.items():
        assert decl in text, name
        assert name in _lib.SYMBOLS and name in _lib.ARGTYPES, name
        fn = getattr(L, name)
        assert fn.restype is C.c_int and fn.argtypes == _lib.ARGTYPES[name] and len(fn.argtypes) == N_ARGS[name], name
    # the descriptor the feeds take is the existing one, and ops_on_device is a plain int
    for name in ("rv_stream_feed_wdev", "rv_eval_stream_feed_wdev"):
        assert _lib.ARGTYPES[name][3] is C.c_int and _lib.ARGTYPES[name][4] is C.POINTER(_lib.DevWitness)


def test_pure_additions_keep_the_abi_version():
    assert _lib.lib().rv_abi_version() == 8


def test_null_arguments_need_no_device():
    L = _lib.lib()
    w = _lib.DevWitness()
    fake = C.c_void_p(0x1000)  # (stands for a handle or device memory: never read when another argument is NULL)
    n = C.c_size_t(77)
    out = C.c_void_p()
    for feed in (L.rv_stream_feed_wdev, L.rv_eval_stream_feed_wdev):
        assert feed(None, None, 0, 0, C.byref(w)) == E_ARG
        assert feed(None, None, 0, 1, None) == E_ARG
        assert feed(None, fake, 5, 1, C.byref(w)) == E_ARG
    for finish in (L.rv_stream_finish_device, L.rv_stream_finish_batch_device):
        assert finish(None, fake, 4096, C.byref(n)) == E_ARG
        assert finish(fake, None, 4096, C.byref(n)) == E_ARG  # (a NULL destination is refused before the handle is looked at)
        assert finish(fake, fake, 4096, None) == E_ARG
    assert L.rv_stream_verify_begin_device(None, 0, 4, fake, 100, 0, C.byref(out)) == E_ARG and not out.value
    assert L.rv_stream_verify_begin_device(fake, 0, 4, None, 100, 0, C.byref(out)) == E_ARG
    assert L.rv_stream_verify_begin_device(fake, 0, 4, fake, 100, 0, None) == E_ARG
    ptrs, lens = (C.c_void_p * 2)(0x1000, 0x2000), (C.c_size_t * 2)(100, 100)
    assert L.rv_stream_verify_begin_batch_device(None, 0, 4, 2, ptrs, lens, 0, C.byref(out)) == E_ARG
    assert L.rv_stream_verify_begin_batch_device(fake, 0, 4, 2, None, lens, 0, C.byref(out)) == E_ARG
    assert L.rv_stream_verify_begin_batch_device(fake, 0, 4, 2, ptrs, None, 0, C.byref(out)) == E_ARG
    assert L.rv_stream_verify_begin_batch_device(fake, 0, 4, 0, ptrs, lens, 0, C.byref(out)) == E_ARG
    assert L.rv_stream_verify_begin_batch_device(fake, 0, 4, 2, (C.c_void_p * 2)(0x1000, 0), lens, 0, C.byref(out)) == E_ARG
    assert L.rv_hook_stream_traffic(None) == E_ARG
    t = (C.c_uint64 * 4)()
    assert L.rv_hook_stream_traffic(t) == 0 and all(x >= 0 for x in t)  # (process-wide counters: other tests may have streamed already)
    assert L.rv_hook_stream_verify_device_paths(None) == E_ARG
    assert L.rv_hook_stream_verify_device_paths((C.c_uint64 * 2)()) == 0
    h, d = C.c_uint64(), C.c_uint64()
    assert L.rv_hook_stream_wit_sums(None, None, 0, 0, None, 0, 0, C.byref(h), C.byref(d)) == E_ARG
    assert L.rv_hook_stream_wit_sums(fake, None, 0, 0, None, 0, 0, None, C.byref(d)) == E_ARG
    assert L.rv_hook_stream_wit_sums(fake, None, 3, 0, None, 0, 0, C.byref(h), C.byref(d)) == E_ARG


def test_python_feeds_refuse_host_side_tensors_before_any_context(monkeypatch):
    torch = pytest.importorskip("torch")
    from reverie_amd import proof, stream

    def no_context(*a, **k):
        raise AssertionError("a context was made before the witness was refused")

    monkeypatch.setattr(proof.Context, "default", classmethod(no_context))
    monkeypatch.setattr(proof.Context, "__init__", no_context)
    ops = np.zeros(0, stream.OP_DTYPE)
    cpu2, cpu64 = torch.zeros(4, dtype=torch.uint8), torch.zeros(2, dtype=torch.int64)
    # a CPU tensor as witness, in either place, through every one-shot function and the helper the classes' feeds call first
    for g, z in ((cpu2, []), ([], cpu64), (cpu2, cpu64), ([0, 1, 0, 1], cpu64)):
        with pytest.raises(TypeError):
            stream.prove_streaming(ops, g, z, (2, 4))
        with pytest.raises(TypeError):
            stream.evaluate_streaming(ops, g, z, (2, 4))
        for batched in (False, True):
            with pytest.raises(TypeError):
                stream._wdev(g, z, None, "feed", batched)
    with pytest.raises(TypeError):
        stream.prove_streaming_batch(ops, torch.zeros((3, 4), dtype=torch.uint8), [], (2, 4))

    # half host, half device: a stand-in for a GPU tensor (no device here) next to host elements
    class OnGpu(torch.Tensor):
        @property
        def device(self):
            return torch.device("cuda", 0)

    gpu2 = torch.zeros(4, dtype=torch.uint8).as_subclass(OnGpu)
    gpu64 = torch.zeros(2, dtype=torch.int64).as_subclass(OnGpu)
    assert gpu2.device.type == "cuda"
    for g, z in ((gpu2, [3, 5]), ([0, 1, 0, 1], gpu64), (gpu2, np.array([3, 5], np.uint64))):
        with pytest.raises(TypeError):
            stream._wdev(g, z, None, "feed", False)
        with pytest.raises(TypeError):
            stream.prove_streaming(ops, g, z, (2, 4))
        with pytest.raises(TypeError):
            stream.evaluate_streaming(ops, g, z, (2, 4))
    # host witnesses pass the check untouched (None: the feed goes the host way, as ever)
    assert stream._wdev([0, 1], [3], None, "feed", False) is None and stream._wdev(np.zeros((2, 3), np.uint8), (), None, "feed", True) is None
