"""rv_bristol_write, the host definition of the Bristol writers (no GPU): its bytes against `reverie_amd.bristol.dumps` (the numpy
writer, which shares no code with it), the round trip through rv_bristol_parse, the error rule case by case, and the per-record code
of reverie_amd/csrc/bristol_write.h -- what the kernels run -- as plain CPU loops in a stand-alone program built with
-fsanitize=address,undefined (tests/bristol_write_asan.cpp): the whole-list pipeline and the windowed rule for every cut."""
import ctypes as C
import os
import re
import struct
import subprocess

import numpy as np
import pytest

import bristol_write_cases as bw
from conftest import ROOT


@pytest.fixture(scope="module")
def L():
    from reverie_amd import _lib

    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__

        __graft_entry__.build()
    return _lib.lib()


def host_write(L, program, n_outputs=0, n_wires=None):
    """-> (code, text)"""
    p = np.ascontiguousarray(program)
    out, n = C.c_void_p(), C.c_size_t()
    rc = L.rv_bristol_write(C.c_void_p(p.ctypes.data) if len(p) else None, C.c_size_t(len(p)), C.c_uint64(n_wires or 0), C.c_uint64(n_outputs),
                            C.byref(out), C.byref(n))
    text = C.string_at(out, n.value) if rc == 0 else None
    if out:
        L.rv_free(out)
    return rc, text


def test_symbols_exported_and_bound(L):
    from reverie_amd import _lib, bristol, program_file

    hdr = open(os.path.join(ROOT, "include", "reverie_amd.h")).read()
    for name in ("rv_bristol_write", "rv_bristol_write_device", "rv_hook_bristol_write_tiles", "rv_bristol_writer_begin", "rv_bristol_writer_feed",
                 "rv_bristol_writer_finish", "rv_bristol_writer_destroy", "rv_program_writer_begin", "rv_program_writer_feed", "rv_program_writer_finish",
                 "rv_program_writer_destroy"):
        assert name in _lib.SYMBOLS and name in _lib.ARGTYPES
        assert getattr(L, name).argtypes is not None
        assert re.search(r"\b" + name + r"\s*\(", hdr), name
    assert C.sizeof(_lib.WriterPiece) == 32
    assert L.rv_abi_version() == 8  # (calls were added, nothing changed)
    out = (C.c_uint32 * 2)()
    assert L.rv_hook_bristol_write_tiles(out) == 0 and L.rv_hook_bristol_write_tiles(None) == bw.ARG
    assert out[0] == 256 and out[1] >= out[0]
    for f in (bristol.dumps_device, bristol.DeviceWriter, bristol.write_device, program_file.DeviceWriter, program_file.write_device):
        assert callable(f)


@pytest.mark.parametrize("name,program,n_outputs,n_wires", bw.ok_cases(), ids=[c[0] for c in bw.ok_cases()])
def test_bytes_are_dumps_bytes(L, name, program, n_outputs, n_wires):
    want = bw.expect(program, n_outputs, n_wires)
    assert want is not None
    assert host_write(L, program, n_outputs, n_wires) == (0, want)
    if n_wires is None:  # the derived count, stated: the same bytes
        assert host_write(L, program, n_outputs, bw.derived(program)[1] or None) == (0, want)


def test_line_kinds_and_lengths(L):
    """the model itself, pinned once: the five lines, the shortest (11 bytes) and the longest (41)"""
    rc, text = host_write(L, bw.prog(bw.inputs(2) + [bw.XOR(2, 0, 1), bw.AND(3, 2, 1), bw.INV(4, 3), bw.EQW(5, 4), bw.EQ(6, 1)]), 2)
    assert rc == 0 and text == b"5 7\n1 2\n1 2\n\n2 1 0 1 2 XOR\n2 1 2 1 3 AND\n1 1 3 4 INV\n1 1 4 5 EQW\n1 1 1 6 EQ\n"
    rc, text = host_write(L, bw.prog([bw.SHORTEST, bw.LONGEST]))
    lines = text.split(b"\n\n", 1)[1].split(b"\n")
    assert [len(ln) + 1 for ln in lines[:2]] == [11, 41] and lines[1] == b"2 1 4294967294 4294967293 4294967295 XOR"


def test_round_trip_through_the_parser(L):
    from reverie_amd import bristol

    for seed in range(6):
        p = bw.random_program(1 + seed, 50 + 7 * seed, 100 + seed)
        rc, text = host_write(L, p, min(2, len(p)))
        assert rc == 0
        back, info = bristol.parse(text)
        assert back.tobytes() == p.tobytes() and info["n_outputs"] == min(2, len(p))


@pytest.mark.parametrize("name,program,n_outputs,n_wires,code", bw.bad_cases(), ids=[c[0] for c in bw.bad_cases()])
def test_codes(L, name, program, n_outputs, n_wires, code):
    assert host_write(L, program, n_outputs, n_wires) == (code, None)
    assert bw.expect(program, n_outputs, n_wires) is None  # the model refuses the list too


def test_argument_errors(L):
    out, n = C.c_void_p(), C.c_size_t()
    p = bw.prog(bw.inputs(1))
    assert L.rv_bristol_write(C.c_void_p(p.ctypes.data), C.c_size_t(1), C.c_uint64(0), C.c_uint64(0), None, C.byref(n)) == bw.ARG
    assert L.rv_bristol_write(C.c_void_p(p.ctypes.data), C.c_size_t(1), C.c_uint64(0), C.c_uint64(0), C.byref(out), None) == bw.ARG
    assert L.rv_bristol_write(None, C.c_size_t(1), C.c_uint64(0), C.c_uint64(0), C.byref(out), C.byref(n)) == bw.ARG
    # decided before anything else: bad records do not change it
    bad = bw.bad_cases()[0][1]
    assert L.rv_bristol_write(C.c_void_p(bad.ctypes.data), C.c_size_t(len(bad)), C.c_uint64(0), C.c_uint64(0), None, None) == bw.ARG


def test_model_under_sanitizers(L, tmp_path):
    """the stand-alone program: clean under AddressSanitizer and UBSan; for every case the kernels' order of work gives the host
    writer's code and bytes (the program compares), those are `dumps`' (compared here, by digest), and so does every cutting"""
    exe = str(tmp_path / "bristol_write_asan")
    csrc = os.path.join(ROOT, "reverie_amd", "csrc")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", csrc,
                           os.path.join(ROOT, "tests", "bristol_write_asan.cpp"), os.path.join(csrc, "bristol.cpp"), "-o", exe])
    T = 256
    big = [("tile-%d" % n, bw.random_program(3, n - 3, n), 1, None) for n in (T - 1, T, T + 1, 2 * T + 1)]
    ends = bw.prog(bw.inputs(2) + ([bw.LONGEST] * (T - 3) + [bw.SHORTEST, bw.SHORTEST] + [bw.LONGEST] * (T - 2) + [bw.SHORTEST, bw.LONGEST]))
    whole = [(n, p, o, w, 0) for n, p, o, w in bw.ok_cases() + big + [("tile-ends", ends, 0, None)]] + bw.bad_cases()
    paths, small = [], []
    for k, (name, program, n_outputs, n_wires, code) in enumerate(whole):
        path = str(tmp_path / f"{k:03d}-{name}.ops")
        with open(path, "wb") as f:
            f.write(struct.pack("<QQQ", n_wires or 0, n_outputs, len(program)) + program.tobytes())
        (small if len(program) <= 48 else paths).append(path)
    run = subprocess.run([exe] + paths + ["--cuts"] + small, capture_output=True, text=True)
    assert run.returncode == 0 and "Sanitizer" not in run.stderr and "runtime error" not in run.stderr, (run.stdout[-2000:], run.stderr[-2000:])
    lines = run.stdout.split("\n")
    assert lines[-2] == "bad 0"
    answers = {ln.split()[0]: ln.split()[1:] for ln in lines if re.match(r"\d\d\d-", ln)}
    assert len(answers) == len(whole)
    for k, (name, program, n_outputs, n_wires, code) in enumerate(whole):
        rc, n_bytes, digest = answers[f"{k:03d}-{name}.ops"]
        want = bw.expect(program, n_outputs, n_wires)
        assert int(rc) == code and (want is None) == (code != 0), name
        if want is not None:
            assert int(n_bytes) == len(want) and int(digest, 16) == bw.fnv(want), name
    cuts = [int(ln.split()[1]) for ln in lines if ln.startswith("cuts ")]
    sizes = [len(p) for _, p, _, _, _ in whole if len(p) <= 48]
    assert cuts == [(n + 1) * (n + 2) // 2 for n in sizes] and max(sizes) >= 40  # every pair of cut points of every small case
