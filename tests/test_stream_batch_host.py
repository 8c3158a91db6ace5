"""Batches over one stream, host side (no GPU): the C-ABI additions, their argument checks and the Python surface."""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = open(os.path.join(ROOT, "include", "reverie_amd.h")).read()
NEW = ("rv_stream_begin_batch", "rv_stream_commit_batch", "rv_stream_finish_batch", "rv_prove_streaming_batch", "rv_stream_verify_begin_batch",
       "rv_stream_verify_finish_batch", "rv_verify_streaming_batch")


@pytest.fixture(scope="module")
def L():
    from reverie_amd import _lib

    return _lib.lib()


def _n_params(name):
    decl = re.search(r"\bint " + name + r"\((.*?)\);", HDR, re.S).group(1)
    decl = re.sub(r"/\*.*?\*/", "", decl, flags=re.S)
    return len([p for p in decl.split(",") if p.strip()])


def test_new_symbols_declared_exported_and_typed(L):
    from reverie_amd import _lib

    declared = set(re.findall(r"\b(rv_[a-z0-9_]+)\s*\(", HDR))
    for name in NEW:
        assert name in declared and name in _lib.SYMBOLS
        fn = getattr(L, name)
        assert fn.restype is C.c_int
        assert fn.argtypes is not None and len(fn.argtypes) == _n_params(name), name


def test_null_arguments_and_empty_batch(L):
    # (no device needed: every null handle or array, and batch == 0, is refused before a context is looked at)
    h = C.c_void_p()
    assert L.rv_stream_begin_batch(None, 0, 4, 2, None, 0, C.byref(h)) == 9
    assert L.rv_stream_begin_batch(None, 0, 4, 0, None, 0, C.byref(h)) == 9
    assert L.rv_stream_begin_batch(None, 0, 4, 2, None, 0, None) == 9
    assert not h.value
    assert L.rv_stream_commit_batch(None, None) == 9
    assert L.rv_stream_finish_batch(None, None, None) == 9
    outs, lens = (C.c_void_p * 2)(), (C.c_size_t * 2)()
    assert L.rv_stream_finish_batch(None, outs, lens) == 9
    assert L.rv_prove_streaming_batch(None, None, 0, 0, 4, 2, None, 0, None, 0, None, 0, outs, lens, None) == 9
    assert L.rv_prove_streaming_batch(None, None, 0, 0, 4, 0, None, 0, None, 0, None, 0, outs, lens, None) == 9
    ptrs, plens = (C.c_void_p * 2)(), (C.c_size_t * 2)()
    assert L.rv_stream_verify_begin_batch(None, 0, 4, 2, ptrs, plens, 0, C.byref(h)) == 9
    assert L.rv_stream_verify_begin_batch(None, 0, 4, 2, None, None, 0, C.byref(h)) == 9
    assert L.rv_stream_verify_begin_batch(None, 0, 4, 0, ptrs, plens, 0, C.byref(h)) == 9
    assert not h.value
    ok = (C.c_int * 2)()
    assert L.rv_stream_verify_finish_batch(None, 0, ok) == 9
    assert L.rv_stream_verify_finish_batch(None, 0, None) == 9
    assert L.rv_verify_streaming_batch(None, None, 0, 0, 4, 2, ptrs, plens, 0, 0, ok, None) == 9
    assert L.rv_verify_streaming_batch(None, None, 0, 0, 4, 0, ptrs, plens, 0, 0, ok, None) == 9


def test_abi_version_unchanged(L):
    assert L.rv_abi_version() == 8  # (a pure addition)


def test_python_surface():
    import reverie_amd
    from reverie_amd import stream

    assert callable(reverie_amd.prove_streaming_batch) and callable(reverie_amd.verify_streaming_batch)
    assert {"feed", "same_cuts", "commit", "finish", "info", "close"} <= set(dir(reverie_amd.StreamingBatchProver))
    assert {"feed", "finish", "info", "close"} <= set(dir(reverie_amd.StreamingBatchVerifier))
    assert stream.prove_streaming_batch is reverie_amd.prove_streaming_batch


def test_witness_rows_must_match_the_batch():
    """a witness array whose first dimension is not the batch is refused before anything reaches the library"""
    from reverie_amd.stream import StreamingBatchProver, prove_streaming_batch

    sp = StreamingBatchProver.__new__(StreamingBatchProver)  # (no context: feed checks the witness shapes first)
    sp.batch, sp.handle = 3, C.c_void_p()
    ops = [(0, 0, 0, 0, 0, 0, 0)]
    with pytest.raises(ValueError):
        sp.feed(ops, np.zeros((2, 1), np.uint8))
    with pytest.raises(ValueError):
        sp.feed(ops, np.zeros((3, 1), np.uint8), np.zeros((4, 1), np.uint64))
    with pytest.raises(ValueError):
        sp.feed(ops, np.zeros(1, np.uint8))  # (1-D is one witness: batch 1 only)
    with pytest.raises(ValueError):
        prove_streaming_batch(ops, np.zeros(1, np.uint8), [], (0, 1), ctx=object())
    with pytest.raises(ValueError):
        prove_streaming_batch(ops, np.zeros((2, 1), np.uint8), np.zeros((3, 1), np.uint64), (1, 1), ctx=object())
