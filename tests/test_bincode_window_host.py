"""The windowed program-file reader (rv_program_reader_*), the part that needs no GPU: the symbols, the command line's flags, and
the reader's state machine between the windows (reverie_amd/csrc/bincode_dev.h: bc_window_*, bc_enter, and the tile walk, map
composition and decode under them -- what the library runs) as plain CPU loops in a stand-alone program built with
-fsanitize=address,undefined (tests/bincode_window_model.cpp).  Every window is a heap block of exactly its bytes; records, per-feed
counts and the first code are compared with rv_program_from_bincode for every case file cut into two windows, the small files fed
1, 31, 32 and 33 bytes at a time, 2 000 seeded random byte mutations at random cuts, and readers placed above 2^32.

Two windows at every position is what files up to 13 000 bytes get: every defect, truncation, ordering and header case, the 32
entry-offset cases and the boundary cases of one to three tiles.  A cut costs a pass over the whole file, so the files of one and
two scan blocks (1 and 2 MiB) are cut at every position within 5 bytes of their two ends and of the first tile boundary, around
the first scan block's end, and at seeded random positions."""
import ctypes as C
import os
import re
import subprocess

import pytest

from conftest import ROOT

NEW = ("rv_program_reader_begin", "rv_program_reader_feed", "rv_program_reader_finish", "rv_program_reader_destroy", "rv_hook_program_reader_resume")


@pytest.fixture(scope="module")
def L():
    from reverie_amd import _lib

    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__

        __graft_entry__.build()
    return _lib.lib()


def test_symbols_exported_and_bound(L):
    from reverie_amd import _lib, program_file, stream

    hdr = open(os.path.join(ROOT, "include", "reverie_amd.h")).read()
    for name in NEW:
        assert name in _lib.SYMBOLS and name in _lib.ARGTYPES
        assert getattr(L, name).argtypes is not None
        assert getattr(L, name).restype is (None if name.endswith("destroy") else C.c_int)
        assert re.search(r"\b" + name + r"\s*\(", hdr), name
    assert C.sizeof(_lib.ProgramPiece) == 32
    body = re.search(r"typedef struct rv_program_piece \{(.*?)\} rv_program_piece;", hdr, re.S).group(1)
    assert re.findall(r"\b([a-z0-9_]+)\s*[,;]", re.sub(r"/\*.*?\*/", "", body, flags=re.S)) == [n for n, _ in _lib.ProgramPiece._fields_]
    assert L.rv_abi_version() == 8  # (calls were added, nothing changed)
    for fn in (program_file.DeviceReader, program_file.iter_device, program_file.scan_device, stream.prove_streaming_pieces,
               stream.verify_streaming_pieces, stream.evaluate_streaming_pieces):
        assert callable(fn)
    # argument errors that need no context
    assert L.rv_program_reader_begin(None, 8, None) == 9 and L.rv_program_reader_finish(None, None) == 9
    assert L.rv_program_reader_feed(None, None, 0, 0, None, 0, None) == 9 and L.rv_hook_program_reader_resume(None, 0, 0) == 9
    L.rv_program_reader_destroy(None)


def test_cli_flags(capsys):
    from reverie_amd.__main__ import build_parser, main

    paths = ["--program-path", "none.bin", "--witness-path", "none.txt", "--proof-path", "none.proof"]
    for mb in ("0", "-1", "4096"):
        with pytest.raises(SystemExit) as e:
            main(["--operation", "prove", "--stream", "--window-mb", mb] + paths)
        assert e.value.code == 2 and "--window-mb" in capsys.readouterr().err
    with pytest.raises(SystemExit) as e:
        main(["--operation", "oneshot", "--stream"] + paths)
    assert e.value.code == 2 and "--evaluator stream" in capsys.readouterr().err
    a = build_parser().parse_args(["--operation", "verify", "--stream", "--window-mb", "4"])
    assert a.stream and a.window_mb == 4
    a = build_parser().parse_args(["--operation", "verify"])
    assert not a.stream and a.window_mb is None
    assert "parsed whole" in " ".join(build_parser().format_help().split())


def test_pieces_of_host_arrays_count_their_inputs():
    import numpy as np

    from reverie_amd import stream
    from reverie_amd.ops import GF2, Z64, program

    prog = program([GF2.Input(0), Z64.Input(0), GF2.Input(1), GF2.Add(2, 0, 1), Z64.Const(1, 0)])
    assert stream._piece_inputs(prog, None) == (2, 1) and stream._piece_inputs(prog, (5, 6)) == (5, 6)
    assert stream._piece_inputs(prog, {"n_input_gf2": 3, "n_input_z64": 4}) == (3, 4)
    fed = []
    pieces = lambda: iter([(prog[:2], None), (prog[:0], None), (prog[2:], None)])  # noqa: E731
    stream._feed_pieces(lambda ops, g, z: fed.append((len(ops), g.tolist(), z.tolist())), pieces, np.array([1, 0], np.uint8), np.array([7], np.uint64))
    assert fed == [(2, [1], [7]), (3, [0], [])]
    with pytest.raises(TypeError):
        stream.prove_streaming_pieces(iter([]), [], [], (0, 0))


def test_model_under_sanitizers(L, tmp_path):
    """the stand-alone program: clean under AddressSanitizer and UBSan, and for every input and every cut the host reader's
    records, per-feed counts and code"""
    import bincode_cases as bc

    exe = str(tmp_path / "bincode_window_model")
    csrc = os.path.join(ROOT, "reverie_amd", "csrc")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", csrc,
                           os.path.join(ROOT, "tests", "bincode_window_model.cpp"), os.path.join(csrc, "program.cpp"), "-o", exe])
    files, small = {}, []
    for k, (name, data) in enumerate(bc.all_files()):
        path = str(tmp_path / f"{k:03d}-{name}.bin")
        open(path, "wb").write(data)
        files[name] = path
        if len(data) <= 1100:
            small.append(path)
    assert len(small) >= 80
    run = subprocess.run([exe] + list(files.values()) + ["--fixed"] + small + [files["every-kind"], "--mutations", "2000", files["3T+1"], "--resume",
                         files["every-kind"]], capture_output=True, text=True)
    assert run.returncode == 0 and "Sanitizer" not in run.stderr and "runtime error" not in run.stderr, (run.stdout[-2000:], run.stderr[-2000:])
    lines = run.stdout.split("\n")
    assert lines[-2] == "bad 0" and "mutations 2000" in lines and "resume 2" in lines
    assert sum(ln.startswith("cuts ") for ln in lines) == len(files) + len(small) + 2 and sum(ln.startswith("fixed ") for ln in lines) == len(small) + 2
    # every cut for the files that are short enough: the count says so
    cuts = [int(ln.split()[1]) for ln in lines if ln.startswith("cuts ")][:len(files)]
    for (name, data), n in zip(bc.all_files(), cuts):
        assert n == len(data) + 1 or len(data) > 13000, name
