"""Streaming cleartext evaluation, host side (no GPU): the C-ABI additions, their argument checks and the CLI switch."""
import ctypes as C
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = open(os.path.join(ROOT, "include", "reverie_amd.h")).read()
NEW = ("rv_eval_stream_begin", "rv_eval_stream_feed", "rv_eval_stream_finish", "rv_eval_stream_get_info", "rv_eval_stream_abort",
       "rv_evaluate_streaming")


@pytest.fixture(scope="module")
def L():
    from reverie_amd import _lib

    return _lib.lib()


def test_new_symbols_exported_and_typed(L):
    from reverie_amd import _lib

    declared = set(re.findall(r"\b(rv_[a-z0-9_]+)\s*\(", HDR))
    for name in NEW:
        assert name in declared and name in _lib.SYMBOLS
        assert getattr(L, name).restype is (None if name == "rv_eval_stream_abort" else C.c_int)
    body = re.search(r"typedef struct rv_eval_stream_info \{(.*?)\} rv_eval_stream_info;", HDR, re.S).group(1)
    fields = [f for line in re.findall(r"uint64_t ([^;]+);", body) for f in re.split(r"\s*,\s*", line)]
    assert fields == [n for n, _ in _lib.EvalStreamInfo._fields_]
    assert fields == ["n_ops", "chunks", "levels", "wire_store_bytes", "peak_chunk_bytes"]
    assert C.sizeof(_lib.EvalStreamInfo) == 40


def test_null_arguments(L):
    # (no device needed: every null handle is refused before a context is looked at)
    h = C.c_void_p()
    assert L.rv_eval_stream_begin(None, C.c_size_t(0), C.c_size_t(4), C.c_size_t(1), C.c_size_t(0), C.byref(h)) == 9
    assert not h.value
    assert L.rv_eval_stream_feed(None, None, C.c_size_t(0), None, C.c_size_t(0), None, C.c_size_t(0)) == 9
    assert L.rv_eval_stream_finish(None, None, None, None) == 9
    assert L.rv_eval_stream_get_info(None, None) == 9
    L.rv_eval_stream_abort(None)
    assert L.rv_evaluate_streaming(None, None, C.c_size_t(0), C.c_size_t(0), C.c_size_t(0), C.c_size_t(1), None, C.c_size_t(0), None,
                                   C.c_size_t(0), C.c_size_t(0), None, None, None, None) == 9


def test_abi_version_unchanged(L):
    assert L.rv_abi_version() == 8  # (a pure addition)


def test_cli_accepts_the_stream_evaluator():
    from reverie_amd.__main__ import build_parser

    a = build_parser().parse_args(["--operation", "oneshot", "--evaluator", "stream", "--max-chunk-ops", "4096", "--program-path", "p.rvops",
                                   "--witness-path", "w.txt"])
    assert a.evaluator == "stream" and a.max_chunk_ops == 4096
    a = build_parser().parse_args(["--operation", "oneshot", "--program-path", "p", "--witness-path", "w"])
    assert a.evaluator == "auto" and a.max_chunk_ops == 0


def test_python_surface():
    import reverie_amd

    assert callable(reverie_amd.evaluate_streaming)
    assert {"feed", "finish", "info", "close"} <= set(dir(reverie_amd.StreamingEvaluator))
