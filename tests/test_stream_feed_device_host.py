"""Streams fed from device memory -- what holds without a GPU: the entry points are declared in the header, exported by the library
and bound in _lib.py, they are pure additions (the ABI version stays 8), and the argument checks answer before any device is
touched."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from reverie_amd import _lib

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "reverie_amd.h")
NEW = {
    "rv_stream_feed_device": "int rv_stream_feed_device(rv_stream *s, const rv_op *d_ops, size_t n_ops, const uint8_t *wit_gf2, size_t n_gf2, "
                             "const uint64_t *wit_z64, size_t n_z64);",
    "rv_eval_stream_feed_device": "int rv_eval_stream_feed_device(rv_eval_stream *s, const rv_op *d_ops, size_t n_ops, const uint8_t *wit_gf2, "
                                  "size_t n_gf2, const uint64_t *wit_z64, size_t n_z64);",
    "rv_hook_stream_op_traffic": "int rv_hook_stream_op_traffic(uint64_t out[2]);",
    "rv_hook_stream_piece_sums": "int rv_hook_stream_piece_sums(rv_ctx *ctx, const rv_op *ops, size_t n_ops, uint64_t first_index, size_t piece_ops, "
                                 "uint64_t *host_out, uint64_t *dev_out);",
}


def test_declared_exported_and_bound():
    text = re.sub(r"\s+", " ", open(HEADER).read())
    L = _lib.lib()
    for name, decl in NEW.items():
        assert decl in text, name
        assert name in _lib.SYMBOLS and name in _lib.ARGTYPES, name
        fn = getattr(L, name)
        assert fn.restype is C.c_int and fn.argtypes == _lib.ARGTYPES[name], name
    assert len(_lib.ARGTYPES["rv_stream_feed_device"]) == 7 and len(_lib.ARGTYPES["rv_eval_stream_feed_device"]) == 7


def test_pure_additions_keep_the_abi_version():
    assert _lib.lib().rv_abi_version() == 8


def test_argument_checks_need_no_device():
    L = _lib.lib()
    E_ARG = 9
    for feed in (L.rv_stream_feed_device, L.rv_eval_stream_feed_device):
        # a NULL stream, with and without an op pointer (the pointer is never read: it is not device memory)
        assert feed(None, None, 0, None, 0, None, 0) == E_ARG
        assert feed(None, None, 5, None, 0, None, 0) == E_ARG
        assert feed(None, C.c_void_p(0x1000), 5, None, 0, None, 0) == E_ARG
    assert L.rv_hook_stream_op_traffic(None) == E_ARG
    out = (C.c_uint64 * 2)()
    assert L.rv_hook_stream_op_traffic(out) == 0
    assert out[0] >= 0 and out[1] >= 0  # (process-wide counters: other tests may have streamed already)
    h, d = (C.c_uint64 * 8)(), (C.c_uint64 * 8)()
    assert L.rv_hook_stream_piece_sums(None, None, 0, 0, 0, h, d) == E_ARG


def test_python_feeds_refuse_host_tensors_before_any_context():
    torch = pytest.importorskip("torch")
    from reverie_amd import proof, stream

    t = torch.zeros((4, 24), dtype=torch.uint8)
    assert proof._is_device_ops(t) and not proof._is_device_ops(np.zeros((4, 24), np.uint8))
    with pytest.raises(TypeError):
        proof._device_ops(t, None, "a feed of device ops")
    with pytest.raises(TypeError):
        stream.prove_streaming(t, [], [], (0, 4))
