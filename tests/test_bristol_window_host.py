"""The windowed Bristol reader (rv_bristol_reader_*), the part that needs no GPU: the symbols, the command line's flags,
rv_bristol_header_prefix, and the reader between the windows (reverie_amd/csrc/bristol_dev.h: what a lane, a line and the state
machine br_window_* do -- what the library runs) as plain CPU loops in a stand-alone program built with
-fsanitize=address,undefined (tests/bristol_window_model.cpp).  Every window and every carry is a heap block of exactly its bytes;
records, per-feed line counts, the feed a code arrives with and the info are compared with rv_bristol_parse for every text of
bristol_cases with and without expected outputs, cut in two (texts up to 2100 bytes at every position, longer ones near both ends,
the header's end and every 4096-byte tile edge, and at seeded positions), the small texts fed 1, 7, 8 and 9 bytes at a time, 1500
seeded byte mutations at random cuts, and a reader placed above 2^32."""
import ctypes as C
import os
import re
import struct
import subprocess

import numpy as np
import pytest

from conftest import ROOT

NEW = ("rv_bristol_header_prefix", "rv_bristol_reader_begin", "rv_bristol_reader_feed", "rv_bristol_reader_header", "rv_bristol_reader_finish",
       "rv_bristol_reader_destroy", "rv_hook_bristol_reader_resume")


@pytest.fixture(scope="module")
def L():
    from reverie_amd import _lib

    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__

        __graft_entry__.build()
    return _lib.lib()


def test_symbols_exported_and_bound(L):
    from reverie_amd import _lib, bristol

    hdr = open(os.path.join(ROOT, "include", "reverie_amd.h")).read()
    for name in NEW:
        assert name in _lib.SYMBOLS and name in _lib.ARGTYPES
        assert getattr(L, name).argtypes is not None
        assert getattr(L, name).restype is (None if name.endswith("destroy") else C.c_int)
        assert re.search(r"\b" + name + r"\s*\(", hdr), name
    assert C.sizeof(_lib.BristolPiece) == 40
    body = re.search(r"typedef struct rv_bristol_piece \{(.*?)\} rv_bristol_piece;", hdr, re.S).group(1)
    assert re.findall(r"\b([a-z0-9_]+)\s*[,;]", re.sub(r"/\*.*?\*/", "", body, flags=re.S)) == [n for n, _ in _lib.BristolPiece._fields_]
    assert L.rv_abi_version() == 8  # (calls were added, nothing changed)
    for fn in (bristol.DeviceReader, bristol.iter_device, bristol.wire_counts):
        assert callable(fn)
    # argument errors that need no context
    assert L.rv_bristol_reader_begin(None, 8, 0, None, 0, None) == 9 and L.rv_bristol_reader_finish(None, None) == 9
    assert L.rv_bristol_reader_feed(None, None, 0, 0, None, 0, None) == 9 and L.rv_hook_bristol_reader_resume(None, 0, 0, 0) == 9
    assert L.rv_bristol_reader_header(None, None) == 9 and L.rv_bristol_header_prefix(None, 0, 0, 0, None, None) == 9
    L.rv_bristol_reader_destroy(None)


def test_cli_flags(capsys):
    from reverie_amd.__main__ import build_parser

    a = build_parser().parse_args(["--operation", "prove", "--stream", "--parser", "device", "--window-mb", "64", "--program-format", "bristol"])
    assert a.stream and a.window_mb == 64 and a.parser == "device"
    a = build_parser().parse_args(["--operation", "oneshot", "--evaluator", "stream", "--parser", "device", "--window-mb", "4"])
    assert a.window_mb == 4 and a.evaluator == "stream"
    a = build_parser().parse_args(["--operation", "prove", "--stream", "--parser", "device"])
    assert a.window_mb is None  # (a Bristol file then goes the way it always went: parsed whole)
    text = " ".join(build_parser().format_help().split())
    assert "parsed whole" in text and "Bristol" in text and "read in windows" in text


def _prefix(L, text, n, full, fmt=0):
    from reverie_amd import _lib

    bi, off = _lib.BristolInfo(), C.c_size_t()
    buf = np.frombuffer(text, np.uint8) if len(text) else np.zeros(1, np.uint8)
    rc = L.rv_bristol_header_prefix(C.c_void_p(buf.ctypes.data), C.c_size_t(n), C.c_uint64(full), C.c_int(fmt), C.byref(bi), C.byref(off))
    return rc, {k: int(getattr(bi, k)) for k, _ in bi._fields_} if rc == 0 else None, int(off.value) if rc == 0 else None


def _four_lines(text):
    """the length of the shortest prefix that holds four whole non-blank lines (the whole text when there is none)"""
    lines = 0
    for m in re.finditer(rb"[^\n]*\n", text):
        lines += bool(m.group(0).strip(b" \t\r\n"))
        if lines == 4:
            return m.end()
    return len(text)


def test_header_prefix(L):
    import bristol_cases as bc

    texts = [(n, t, f) for n, t, f in bc.well_formed() + bc.boundary_texts()] + [(n, t, f) for n, t, _, f, _ in bc.error_texts()]
    seen_short = 0
    for name, text, fmt in texts:
        rc, info, off = bc.host_header(text, fmt)
        want = (rc, info if rc == 0 else None, off if rc == 0 else None)
        assert _prefix(L, text, len(text), len(text), fmt) == want, name
        n = _four_lines(text)
        assert _prefix(L, text, n, len(text), fmt) == want, name  # the head, judged with the file's true length
        if rc == 0 and n < len(text) and info["n_gates"] > n // 8 + 1:
            seen_short += 1
            assert bc.host_header(text[:n], fmt)[0] == bc.BAD_OP, name  # (what rv_bristol_header makes of the head alone)
    assert seen_short >= 10
    assert _prefix(L, b"1 2\n", 4, 3)[0] == bc.ARG  # len > full_len


def _case_file(path, text, expected, fmt):
    exp = bytes(expected) if expected is not None else b""
    open(path, "wb").write(struct.pack("<III", fmt, expected is not None, len(exp)) + exp + text)


def test_model_under_sanitizers(L, tmp_path):
    """the stand-alone program: clean under AddressSanitizer and UBSan, and for every text and every cut the host parser's records,
    per-feed line counts, code (with the feed that owes it) and info"""
    import bristol_cases as bc

    exe = str(tmp_path / "bristol_window_model")
    csrc = os.path.join(ROOT, "reverie_amd", "csrc")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", csrc,
                           os.path.join(ROOT, "tests", "bristol_window_model.cpp"), os.path.join(csrc, "bristol.cpp"), "-o", exe])
    cases = []  # (name, text, expected, fmt)
    for name, text, fmt in bc.well_formed() + bc.boundary_texts():
        rc, _, _, info = bc.host_parse(text, None, fmt)
        assert rc == 0, name
        cases.append((name, text, None, fmt))
        cases.append((name + "+exp", text, [(k * 5 + 1) & 1 for k in range(info["n_outputs"])], fmt))
    for name, text, exp, fmt, code in bc.error_texts():
        assert bc.host_parse(text, exp, fmt)[0] == code, name
        cases.append((name, text, exp, fmt))
        if exp is None:
            rc, info, _ = bc.host_header(text, fmt)
            cases.append((name + "+exp", text, [1] * (info["n_outputs"] if rc == 0 else 2), fmt))
    paths, small = {}, []
    for k, (name, text, exp, fmt) in enumerate(cases):
        paths[name] = str(tmp_path / f"{k:03d}.case")
        _case_file(paths[name], text, exp, fmt)
        if len(text) <= 700:
            small.append(paths[name])
    assert len(small) >= 100
    run = subprocess.run([exe] + list(paths.values()) + ["--fixed"] + small + ["--mutations", "1000", paths["fashion+exp"], "--mutations", "500",
                         paths["lines-%d" % (bc.tiles()[1] + 1)], "--resume", paths["fashion+exp"], "--resume", paths["blanks"]], capture_output=True, text=True)
    assert run.returncode == 0 and "Sanitizer" not in run.stderr and "runtime error" not in run.stderr, (run.stdout[-2000:], run.stderr[-2000:])
    lines = run.stdout.split("\n")
    assert lines[-2] == "bad 0" and "mutations 1000" in lines and "mutations 500" in lines and sum(ln.startswith("resume ") for ln in lines) == 2
    cuts = [int(ln.split()[1]) for ln in lines if ln.startswith("cuts ")]
    assert len(cuts) == len(cases) and sum(ln.startswith("fixed 4 ") for ln in lines) == len(small)
    for (name, text, _, _), n in zip(cases, cuts):  # every cut for the texts that are short enough: the count says so
        assert n == len(text) + 1 if len(text) <= 2100 else n >= 40, name
    resumed = sum(int(ln.split()[1]) for ln in lines if ln.startswith("resume "))
    assert int(lines[-3].split()[1]) == sum(cuts) + 4 * len(small) + 1500 + resumed
