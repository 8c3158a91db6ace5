"""rv_program_from_bincode_device / rv_program_to_bincode_device, the part that needs no GPU: the symbols and the struct, the shared
case files against the host reader, and the device reader's own functions (reverie_amd/csrc/bincode_dev.h: the layout table, the tile
walk, the map composition, the record decode -- what the kernels run) as plain CPU loops in a stand-alone program built with
-fsanitize=address,undefined (tests/bincode_walk_asan.cpp), compared with rv_program_from_bincode on every case file, every prefix of
two of them and 2 000 seeded random byte mutations."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT


@pytest.fixture(scope="module")
def L():
    from reverie_amd import _lib

    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__

        __graft_entry__.build()
    return _lib.lib()


def test_symbols_exported_and_bound(L):
    from reverie_amd import _lib, program_file

    hdr = open(os.path.join(ROOT, "include", "reverie_amd.h")).read()
    for name in ("rv_program_from_bincode_device", "rv_program_to_bincode_device", "rv_hook_bincode_tiles"):
        assert name in _lib.SYMBOLS and name in _lib.ARGTYPES
        assert getattr(L, name).argtypes is not None and getattr(L, name).restype is C.c_int
        assert re.search(r"\b" + name + r"\s*\(", hdr), name
    assert C.sizeof(_lib.ProgramInfo) == 64
    body = re.search(r"typedef struct rv_program_info \{(.*?)\} rv_program_info;", hdr, re.S).group(1)
    assert re.findall(r"\b([a-z0-9_]+)\s*[,;]", re.sub(r"/\*.*?\*/", "", body, flags=re.S)) == [n for n, _ in _lib.ProgramInfo._fields_]
    assert L.rv_abi_version() == 8  # (calls were added, nothing changed)
    out = (C.c_uint32 * 2)()
    assert L.rv_hook_bincode_tiles(out) == 0 and L.rv_hook_bincode_tiles(None) == 9
    assert out[0] >= 64 and out[0] % 16 == 0 and out[1] >= 2
    assert callable(program_file.loads_device) and callable(program_file.dumps_device)


def test_case_files_say_what_they_mean(L):
    """the builders' defects are the defects they name: the host reader's code for each (the device tests take the code from the host
    reader too, so a builder that built something else would go unnoticed there)"""
    import bincode_cases as bc

    for name, data, code in bc.single_defect_cases() + bc.ordering_cases():
        assert bc.host_parse(data)[0] == code, name
    for name, data in bc.truncation_cases():
        assert bc.host_parse(data)[0] == bc.BAD_OP, name
    for name, data in bc.header_cases():
        assert bc.host_parse(data)[0] == bc.BAD_OP, name
    for name, data in bc.boundary_cases():
        rc, n, recs = bc.host_parse(data)
        assert rc == (bc.BAD_OP if name.endswith("count+1") else 0), name
        if name.endswith("garbage"):
            assert data.endswith(b"\xff" * 40) and n == bc.count_of(data)
    T, _ = bc.tiles()
    entries = set()
    for e in range(32):
        data = bc.entry_offset_case(e)
        starts, end = bc.record_starts(data)
        assert end == len(data) and bc.host_parse(data)[0] == 0
        entries.add(min(s for s in starts if s >= T) - T)
    assert entries == set(range(32))
    rc, n, recs = bc.host_parse(bc.all_files()[0][1])
    kinds = {(r["domain"], r["opcode"]) for r in np.frombuffer(recs, bc.OP_DTYPE)}
    assert len(kinds) == 22


def test_model_under_sanitizers(L, tmp_path):
    """the stand-alone program: clean under AddressSanitizer and UBSan, and for every input the host reader's code, count, records
    and info"""
    import bincode_cases as bc

    exe = str(tmp_path / "bincode_walk_asan")
    csrc = os.path.join(ROOT, "reverie_amd", "csrc")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", csrc,
                           os.path.join(ROOT, "tests", "bincode_walk_asan.cpp"), os.path.join(csrc, "program.cpp"), "-o", exe])
    files = {}
    for k, (name, data) in enumerate(bc.all_files()):
        path = str(tmp_path / f"{k:03d}-{name}.bin")
        open(path, "wb").write(data)
        files[name] = path
    T, _ = bc.tiles()
    # every prefix of the program of every record kind and of a file a little longer than a tile; mutations of three tiles' worth
    prefixed = [files["every-kind"], str(tmp_path / "tile-and-a-bit.bin")]
    open(prefixed[1], "wb").write(bc.mix_of_length(T + 211, 77))
    run = subprocess.run([exe] + list(files.values()) + ["--mutations", "2000", files["3T+1"], "--prefixes"] + prefixed, capture_output=True, text=True)
    assert run.returncode == 0 and "Sanitizer" not in run.stderr and "runtime error" not in run.stderr, (run.stdout[-2000:], run.stderr[-2000:])
    lines = run.stdout.split("\n")
    assert lines[-2] == "bad 0" and "mutations 2000" in lines
    assert f"prefixes {os.path.getsize(prefixed[0])}" in lines and f"prefixes {os.path.getsize(prefixed[1])}" in lines
    # the program's host-reader answers are the library's
    whole = [ln.split() for ln in lines if re.match(r"\d\d\d-", ln)]
    assert len(whole) == len(files) + 2  # (the mutated and the first prefixed file are case files too)
    for (name, data), (what, n_bytes, rc, n) in zip(bc.all_files(), whole):
        assert what.endswith(name + ".bin") and int(n_bytes) == len(data)
        assert (int(rc), int(n)) == bc.host_parse(data)[:2], name
