"""rv_witness_parse / rv_witness_write, the host definition of the witness text (no GPU): the parser against
`reverie_amd.witness.parse_witness` (the numpy parser, which shares no code with it) on every text of witness_cases, count-only and
with a short capacity; the writer against a three-line Python model; the round trip; the exports; the device calls' refusal without
a GPU; the command line's new switches; and the lane, tile and writer rules of reverie_amd/csrc/witness_text.h -- what the kernels
run -- as plain CPU loops in a stand-alone program built with -fsanitize=address,undefined (tests/witness_text_model.cpp)."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import witness_cases as wc
from conftest import ROOT

NEW = ("rv_witness_parse", "rv_witness_write", "rv_witness_parse_device", "rv_hook_witness_text_tiles", "rv_witness_write_device",
       "rv_witness_reader_begin", "rv_witness_reader_feed", "rv_witness_reader_finish", "rv_witness_reader_destroy")


@pytest.fixture(scope="module")
def L():
    from reverie_amd import _lib

    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__

        __graft_entry__.build()
    return _lib.lib()


@pytest.fixture(scope="module")
def T(L):
    out = (C.c_uint32 * 2)()
    assert L.rv_hook_witness_text_tiles(out) == 0 and L.rv_hook_witness_text_tiles(None) == wc.ARG
    assert out[0] >= 4096 and out[0] % 4096 == 0 and out[1] % 16 == 0
    return int(out[0])


def host_parse(L, text, cap=None, poison=None):
    """-> (code, count, the buffer after the call); cap None: room for every byte; cap -1: count only"""
    t = np.frombuffer(text, np.uint8) if len(text) else np.zeros(1, np.uint8)
    n = C.c_size_t(12345)
    if cap == -1:
        return L.rv_witness_parse(C.c_void_p(t.ctypes.data), C.c_size_t(len(text)), None, C.c_size_t(0), C.byref(n)), n.value, None
    room = len(text) if cap is None else cap
    buf = np.full(room + 1, 0xA5 if poison is None else poison, np.uint8)
    rc = L.rv_witness_parse(C.c_void_p(t.ctypes.data), C.c_size_t(len(text)), C.c_void_p(buf.ctypes.data), C.c_size_t(room), C.byref(n))
    return rc, n.value, buf


def host_write(L, bits, line_bits, cap=None):
    """-> (code, length, the buffer after the call)"""
    b = np.ascontiguousarray(np.asarray(bits, np.uint8))
    n = C.c_size_t(12345)
    p = C.c_void_p(b.ctypes.data) if len(b) else None
    if cap == -1:
        return L.rv_witness_write(p, C.c_size_t(len(b)), C.c_uint64(line_bits), None, C.c_size_t(0), C.byref(n)), n.value, None
    room = 2 * len(b) + 1 if cap is None else cap
    buf = np.full(room + 1, 0xA5, np.uint8)
    rc = L.rv_witness_write(p, C.c_size_t(len(b)), C.c_uint64(line_bits), C.c_void_p(buf.ctypes.data), C.c_size_t(room), C.byref(n))
    return rc, n.value, buf


def test_symbols_exported_and_bound(L, T):
    from reverie_amd import _lib, witness

    hdr = open(os.path.join(ROOT, "include", "reverie_amd.h")).read()
    for name in NEW:
        assert name in _lib.SYMBOLS and name in _lib.ARGTYPES
        assert getattr(L, name).argtypes is not None
        assert getattr(L, name).restype is (None if name.endswith("destroy") else C.c_int)
        assert re.search(r"\b" + name + r"\s*\(", hdr), name
    assert L.rv_abi_version() == 8  # (calls were added, nothing changed)
    for f in (witness.parse_witness, witness.parse, witness.parse_device, witness.dumps, witness.dumps_device, witness.parse_device_batch,
              witness.DeviceReader, witness.DeviceWindows):
        assert callable(f)


def test_device_calls_refuse_without_a_context(L):
    """the code the other device parsers give for a missing context, before anything touches a GPU"""
    n = C.c_size_t()
    t = np.frombuffer(b"0101", np.uint8)
    assert L.rv_bristol_parse_device(None, C.c_void_p(t.ctypes.data), 4, 0, 0, None, 0, None, 0, C.byref(n), None) == wc.ARG
    assert L.rv_witness_parse_device(None, C.c_void_p(t.ctypes.data), 4, 0, None, 0, C.byref(n), None, 0, None) == wc.ARG
    assert L.rv_witness_write_device(None, C.c_void_p(t.ctypes.data), 4, 0, None, 0, C.byref(n)) == wc.ARG
    h = C.c_void_p()
    assert L.rv_witness_reader_begin(None, C.byref(h)) == wc.ARG and not h
    assert L.rv_witness_reader_feed(None, None, 0, 0, None, 0, C.byref(n)) == wc.ARG
    assert L.rv_witness_reader_finish(None, None, None) == wc.ARG
    L.rv_witness_reader_destroy(None)


def test_python_device_faces_raise_without_a_gpu():
    import torch

    from reverie_amd import ReverieError, witness

    if torch.cuda.is_available():
        pytest.skip("GPU present")
    for call in (lambda: witness.parse_device(b"01"), lambda: witness.DeviceReader(), lambda: witness.parse_device_batch([b"0", b"1"])):
        with pytest.raises(ReverieError) as e:
            call()
        assert e.value.code == 7  # (no context without a device: nothing falls back to the host parser)


def test_parse_equals_numpy_parser(L, T):
    from reverie_amd import witness

    seen = 0
    for name, text in wc.texts(T):
        want = witness.parse_witness(text)
        rc, n, buf = host_parse(L, text)
        assert (rc, n) == (0, len(want)) and (buf[:n] == want).all() and (buf[n:] == 0xA5).all(), name
        assert host_parse(L, text, cap=-1)[:2] == (0, len(want)), name
        assert (witness.parse(text) == want).all() and witness.parse(text).dtype == np.uint8, name
        if len(want):  # a short capacity: the count, and not one byte written
            for cap in {0, len(want) // 2, len(want) - 1}:
                rc, n, buf = host_parse(L, text, cap=cap, poison=0x5A)
                assert (rc, n) == (wc.ARG, len(want)) and (buf == 0x5A).all(), (name, cap)
            seen += 1
        rc, n, buf = host_parse(L, text, cap=len(want))  # exactly enough
        assert (rc, n) == (0, len(want)) and (buf[:n] == want).all() and buf[n] == 0xA5, name
    assert seen > 40
    n = C.c_size_t()
    assert L.rv_witness_parse(None, C.c_size_t(3), None, C.c_size_t(0), C.byref(n)) == wc.ARG
    assert L.rv_witness_parse(b"01", C.c_size_t(2), None, C.c_size_t(0), None) == wc.ARG
    assert L.rv_witness_parse(None, C.c_size_t(0), None, C.c_size_t(0), C.byref(n)) == 0 and n.value == 0  # (the empty text)


def test_every_byte_value(L):
    """'0' and '1' alone are bits: all 256 values, one by one and together"""
    for b in range(256):
        rc, n, buf = host_parse(L, bytes([b]))
        assert (rc, n) == (0, 1 if b in (0x30, 0x31) else 0)
        if n:
            assert buf[0] == b - 0x30
    rc, n, buf = host_parse(L, bytes(range(256)))
    assert (rc, n) == (0, 2) and buf[:2].tolist() == [0, 1]
    for b in wc.NEAR_MISSES:
        assert host_parse(L, bytes([b]) * 33)[:2] == (0, 0)


def test_write_equals_model(L, T):
    from reverie_amd import witness

    rng = np.random.default_rng(3)
    for n in (0, 1, 2, 15, 16, 17, 63, 64, 65, 127, 128, 129, T - 1, T, T + 1):
        bits = rng.integers(0, 2, n, dtype=np.uint8)
        for lb in wc.line_bits_values(n):
            want = wc.write_model(bits, lb)
            assert len(want) == (0 if n == 0 else n + (-(-n // lb) if lb else 1)), (n, lb)
            rc, length, buf = host_write(L, bits, lb)
            assert (rc, length) == (0, len(want)) and buf[:length].tobytes() == want and (buf[length:] == 0xA5).all(), (n, lb)
            assert host_write(L, bits, lb, cap=-1)[:2] == (0, len(want)), (n, lb)  # the length only
            rc, length, buf = host_write(L, bits, lb, cap=len(want))  # exactly enough
            assert (rc, length) == (0, len(want)) and buf[:length].tobytes() == want and buf[length] == 0xA5, (n, lb)
            if want:  # too small: the length, nothing written
                rc, length, buf = host_write(L, bits, lb, cap=len(want) - 1)
                assert (rc, length) == (wc.ARG, len(want)) and (buf == 0xA5).all(), (n, lb)
            assert witness.dumps(bits, lb) == want, (n, lb)
            assert (witness.parse(want) == bits).all() and (witness.parse_witness(want) == bits).all(), (n, lb)  # parse(write(x)) == x
    assert wc.write_model([1, 0, 1], 2) == b"10\n1\n" and wc.write_model([1, 0, 1], 0) == b"101\n" and wc.write_model([], 5) == b""
    assert host_write(L, [0, 1], 2 ** 64 - 1)[:2] == (0, 3)  # (a line length no sum may wrap on)


def test_write_refuses_a_byte_above_one(L):
    from reverie_amd import ReverieError, witness

    for n, at in ((1, 0), (40, 0), (40, 39), (40, 17)):
        bits = np.zeros(n, np.uint8)
        bits[at] = 2
        for lb in (0, 7):
            assert host_write(L, bits, lb)[0] == wc.ARG
        bits[at] = 255
        assert host_write(L, bits, 16)[0] == wc.ARG
    with pytest.raises(ReverieError) as e:
        witness.dumps([0, 1, 2])
    assert e.value.code == wc.ARG
    n = C.c_size_t()
    assert L.rv_witness_write(None, C.c_size_t(2), C.c_uint64(0), None, C.c_size_t(0), C.byref(n)) == wc.ARG
    assert L.rv_witness_write(None, C.c_size_t(0), C.c_uint64(0), None, C.c_size_t(0), None) == wc.ARG


def test_cli_switches(capsys):
    from reverie_amd.__main__ import build_parser, main

    a = build_parser().parse_args(["--operation", "prove"])
    assert a.witness_parser == "host" and a.witness_window_mb is None  # no default changes
    a = build_parser().parse_args(["--operation", "prove", "--witness-parser", "device"])
    assert a.witness_parser == "device"
    a = build_parser().parse_args(["--operation", "prove", "--stream", "--witness-parser", "device", "--witness-window-mb", "4"])
    assert a.witness_window_mb == 4
    with pytest.raises(SystemExit):
        build_parser().parse_args(["--operation", "prove", "--witness-parser", "gpu"])
    text = " ".join(build_parser().format_help().split())
    assert "--witness-parser" in text and "--witness-window-mb" in text and "rv_witness_parse_device" in text
    common = ["--program-path", "p.txt", "--witness-path", "w.txt", "--proof-path", "o.bin"]
    bad = [
        (["--operation", "prove", "--witness-window-mb", "4", "--stream"], "needs --witness-parser device"),
        (["--operation", "prove", "--witness-parser", "device", "--witness-window-mb", "4"], "needs a streamed operation"),
        (["--operation", "oneshot", "--witness-parser", "device", "--witness-window-mb", "4", "--evaluator", "gpu"], "needs a streamed operation"),
        (["--operation", "prove", "--stream", "--witness-parser", "device", "--witness-window-mb", "0"], "at least 1"),
        (["--operation", "prove", "--stream", "--witness-parser", "device", "--witness-window-mb", "4096"], "below 4096"),
        (["--operation", "verify", "--witness-parser", "device"], "read a witness"),
        (["--operation", "oneshot", "--witness-parser", "device", "--evaluator", "host"], "--evaluator host cannot read it"),
    ]
    for args, message in bad:
        with pytest.raises(SystemExit) as e:
            main(args + common)
        assert e.value.code == 2 and message in capsys.readouterr().err, args


def test_model_under_sanitizers(L, T, tmp_path):
    """the stand-alone program: clean under AddressSanitizer and UBSan; for every text, every source alignment, every mark and every
    cut of the short texts the kernels' order of work gives the byte loop's bits, and the writer's lanes the byte loop's text (the
    program compares); bits and texts are `parse_witness`' and the Python model's (compared here, by digest)"""
    from reverie_amd import witness

    exe = str(tmp_path / "witness_text_model")
    csrc = os.path.join(ROOT, "reverie_amd", "csrc")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", csrc,
                           os.path.join(ROOT, "tests", "witness_text_model.cpp"), os.path.join(csrc, "witness.cpp"), "-o", exe])
    whole, short = wc.texts(T), wc.short_texts(T)
    assert len(short) >= 30 and max(len(t) for _, t in short) == 40
    paths = {}
    for k, (name, text) in enumerate(whole + short):
        paths[k] = str(tmp_path / f"{k:03d}-{name}.txt")
        open(paths[k], "wb").write(text)
    run = subprocess.run([exe] + [paths[k] for k in range(len(whole))] + ["--cuts"] + [paths[k] for k in range(len(whole), len(paths))],
                         capture_output=True, text=True)
    assert run.returncode == 0 and "Sanitizer" not in run.stderr and "runtime error" not in run.stderr, (run.stdout[-2000:], run.stderr[-2000:])
    lines = run.stdout.split("\n")
    assert lines[-2] == "bad 0" and int(lines[-3].split()[1]) > 30000
    answers = {ln.split()[0]: ln.split()[1:] for ln in lines if re.match(r"\d\d\d-", ln)}
    assert len(answers) == len(paths)
    for k, (name, text) in enumerate(whole + short):
        got = answers[os.path.basename(paths[k])]
        bits = witness.parse_witness(text)
        assert int(got[0]) == len(bits) and int(got[1], 16) == wc.fnv(bits.tobytes()), name
        if len(bits) <= 2 * T + 1:  # (the Python model is a loop: the long texts' writer digests stand on the program's own byte loop)
            assert [int(g, 16) for g in got[2:]] == [wc.fnv(wc.write_model(bits, lb)) for lb in wc.line_bits_values(len(bits))], name
