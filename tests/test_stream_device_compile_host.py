"""Host-side checks of the device compiler's place in the streams (no GPU): the C-ABI additions are exported with the declared
signatures and refuse NULL handles, the ABI version has not moved, the Python classes and one-shot functions take `device_compile`,
and the CLI hands `--compiler device` to the streaming evaluator."""
import ctypes as C
import inspect
import os
import re

import pytest

from conftest import ROOT

NEW = {
    "rv_stream_set_compile_flags": "int rv_stream_set_compile_flags(rv_stream *s, uint32_t flags)",
    "rv_eval_stream_set_compile_flags": "int rv_eval_stream_set_compile_flags(rv_eval_stream *s, uint32_t flags)",
    "rv_hook_compile_compare_device_chunk": "int rv_hook_compile_compare_device_chunk(rv_ctx *ctx, const rv_op *ops, size_t n_ops, size_t z64_wires, "
                                            "size_t gf2_wires, const uint64_t start[6], int *path, int *diff)",
    "rv_hook_stream_device_chunks": "uint64_t rv_hook_stream_device_chunks(void)",
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
        params = sig[sig.index("(") + 1:sig.rindex(")")]
        n_params = 0 if params == "void" else params.count(",") + 1
        assert len(_lib.ARGTYPES[name]) == n_params, name
    assert L.rv_abi_version() == 8  # (pure additions)
    assert L.rv_hook_stream_device_chunks.restype is C.c_uint64
    assert isinstance(L.rv_hook_stream_device_chunks(), int)  # (a process-wide counter: other tests may have streamed already)


def test_null_handles_are_refused(L):
    from reverie_amd import _lib

    for flags in (0, _lib.RV_COMPILE_DEVICE, 8):
        assert L.rv_stream_set_compile_flags(None, flags) == 9
        assert L.rv_eval_stream_set_compile_flags(None, flags) == 9
    path, diff = C.c_int(-1), C.c_int(-1)
    start = (C.c_uint64 * 6)()
    assert L.rv_hook_compile_compare_device_chunk(None, None, 0, 0, 4, start, C.byref(path), C.byref(diff)) == 9


def test_python_surfaces_take_device_compile():
    from reverie_amd import stream

    for name in ("StreamingProver", "StreamingVerifier", "StreamingBatchProver", "StreamingBatchVerifier", "StreamingEvaluator"):
        p = inspect.signature(getattr(stream, name).__init__).parameters
        assert "device_compile" in p and p["device_compile"].default is False, name
    for name in ("prove_streaming", "verify_streaming", "prove_streaming_batch", "verify_streaming_batch", "evaluate_streaming"):
        p = inspect.signature(getattr(stream, name)).parameters
        assert "device_compile" in p and p["device_compile"].default is False, name


@pytest.mark.parametrize("compiler", ["host", "device"])
def test_cli_passes_the_compiler_to_the_streaming_evaluator(monkeypatch, tmp_path, compiler):
    """argument plumbing only: evaluate_stream is replaced, nothing touches a GPU"""
    from reverie_amd import __main__ as cli

    seen = {}

    def fake(program_path, fmt, expected_path, witness, max_chunk_ops, device_compile=False):
        seen.update(program_path=program_path, max_chunk_ops=max_chunk_ops, device_compile=device_compile)

    monkeypatch.setattr(cli, "evaluate_stream", fake)
    wit = tmp_path / "w.txt"
    wit.write_text("101")
    rc = cli.main(["--operation", "oneshot", "--evaluator", "stream", "--compiler", compiler, "--max-chunk-ops", "4096", "--program-path", "p.rvops",
                   "--witness-path", str(wit)])
    assert rc == 0
    assert seen == {"program_path": "p.rvops", "max_chunk_ops": 4096, "device_compile": compiler == "device"}


def test_streaming_evaluator_is_asked_for_the_device_compiler(monkeypatch):
    """evaluate_stream hands device_compile to StreamingEvaluator (a stand-in: no GPU)"""
    import numpy as np

    from reverie_amd import __main__ as cli, stream
    from reverie_amd.ops import GF2, program

    made = {}

    class Fake:
        def __init__(self, wc, batch, max_chunk_ops, device_compile=False):
            made.update(wc=tuple(wc), device_compile=device_compile)

        def feed(self, piece, wit):
            pass

        def finish(self):
            class R:
                ok = [True]

            return R()

        def close(self):
            pass

    monkeypatch.setattr(stream, "StreamingEvaluator", Fake)
    monkeypatch.setattr(cli, "load_program", lambda path, fmt, exp: (program([GF2.Input(0), GF2.AssertZero(1)]), (0, 2)))
    cli.evaluate_stream("x.bristol", "bristol", None, np.array([1], np.uint8), 0, device_compile=True)
    assert made == {"wc": (0, 2), "device_compile": True}
