"""The windowed pruning without a GPU (include/reverie_amd.h: rv_pruner_*, rv_ops_prune_windows_host): the window step
composes to the backward sweep for every way of cutting a list -- in a Python model that goes in the device's order of work
(tests/prune_window_ref.py), in the host function, and in the per-record code of reverie_amd/csrc/prune.h run as plain CPU loops in
a stand-alone program built with -fsanitize=address,undefined (tests/prune_window_model.cpp)."""
import ctypes as C
import os
import re
import struct
import subprocess

import numpy as np
import pytest

import prune_cases as pc
import prune_ref
import prune_window_ref as pw
from conftest import ROOT
from reverie_amd.ops import GF2, OP_DTYPE, program

MAX_OPS = 6000


@pytest.fixture(scope="module")
def L():
    from reverie_amd import _lib

    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__

        __graft_entry__.build()
    return _lib.lib()


@pytest.fixture(scope="module")
def lists(L):
    """the corpus up to 6 000 ops and 120 generated lists, each with its cuttings and the sweep model's (keep flags, info) -- for a
    library that has the windowed calls the model stands for"""
    assert hasattr(L, "rv_ops_prune_windows_host") and hasattr(L, "rv_pruner_mark")
    out = []
    rng = np.random.default_rng(2308)
    for case in [c for c in pc.corpus() if len(c[1]) <= MAX_OPS] + pc.generated(120):
        name, ops, wc, og, oz = case
        out.append((case, pw.cuttings(len(ops), rng), prune_ref.sweep(ops, og, oz)))
    return out


def test_cuttings_are_the_issue_s(lists):
    assert len(lists) >= 190
    kinds = set()
    for (name, ops, *_), cuts, _ in lists:
        n = len(ops)
        assert cuts[0] == []
        for c in cuts:
            assert c == sorted(c) and all(0 <= x <= n for x in c)
            if n >= 2 and c == sorted({1, n - 1}):
                kinds.add("ends")
            if 256 in c and 257 in c:
                kinds.add("tile")
            if 1 < n < 15 and c == list(range(1, n)):
                kinds.add("all")
    assert kinds == {"ends", "tile", "all"}
    assert sum(len(cuts) for _, cuts, _ in lists) > 700


def test_model_composes_to_the_sweep(lists):
    """the window step in the device's order, over every cutting: the sweep's keep flags, class counts and unread-Input counts; on a
    single window the layers are the peeling model's"""
    for (name, ops, wc, og, oz), cuts, (want_keep, want_info) in lists:
        for c in cuts:
            keep, info = pw.prune_windows(ops, c, og, oz)
            assert (keep == want_keep).all(), (name, c)
            for k in prune_ref.CLASSES + ("n_kept", "n_dropped"):
                assert info[k] == want_info[k], (name, c, k)
            if not c:
                assert info["device_rounds"] == prune_ref.peel(ops, og, oz)[1]["device_rounds"], name


def windows_host(L, ops, wc, og, oz, cuts, cap=None):
    """rv_ops_prune_windows_host through ctypes -> (code, records, old_index, info dict, n_out); both buffers padded and the pad checked"""
    from reverie_amd import _lib

    ops = np.ascontiguousarray(ops)
    g, z, c = np.asarray(og, np.uint32), np.asarray(oz, np.uint32), np.asarray(cuts, np.uint64)
    assert C.sizeof(C.c_size_t) == 8
    pi, n_out = _lib.PruneInfo(), C.c_size_t(12345)
    cap = len(ops) if cap is None else cap
    buf = np.full((cap + 1) * 24, 0xA5, np.uint8).view(OP_DTYPE)
    old = np.full(cap + 1, 0xA5A5A5A5, np.uint32)
    p = lambda a: a.ctypes.data_as(C.c_void_p) if a.size else None
    rc = L.rv_ops_prune_windows_host(p(ops), len(ops), int(wc[0]), int(wc[1]), p(g), g.size, p(z), z.size, p(c), c.size, p(buf), cap, C.byref(n_out),
                                     p(old), C.byref(pi))
    assert (buf[cap:].view(np.uint8) == 0xA5).all() and old[cap] == 0xA5A5A5A5
    return rc, buf[:cap], old[:cap], {n: int(getattr(pi, n)) for n, _ in pi._fields_}, int(n_out.value)


def whole_host(L, ops, wc, og, oz):
    from reverie_amd import _lib

    ops = np.ascontiguousarray(ops)
    g, z = np.asarray(og, np.uint32), np.asarray(oz, np.uint32)
    pi, n_out = _lib.PruneInfo(), C.c_size_t(0)
    buf, old = np.zeros(len(ops) + 1, OP_DTYPE), np.zeros(len(ops) + 1, np.uint32)
    p = lambda a: a.ctypes.data_as(C.c_void_p) if a.size else None
    rc = L.rv_ops_prune(p(ops), len(ops), int(wc[0]), int(wc[1]), p(g), g.size, p(z), z.size, p(buf), len(ops), C.byref(n_out), p(old), C.byref(pi))
    k = int(n_out.value)
    return rc, buf[:k], old[:k], {n: int(getattr(pi, n)) for n, _ in pi._fields_}


def test_symbols_and_struct(L):
    import reverie_amd
    from reverie_amd import _lib, prune

    hdr = open(os.path.join(ROOT, "include", "reverie_amd.h")).read()
    names = ("rv_ops_prune_windows_host", "rv_pruner_begin", "rv_pruner_scan", "rv_pruner_scan_end", "rv_pruner_mark", "rv_pruner_mark_end",
             "rv_pruner_feed", "rv_pruner_rewind", "rv_pruner_get_info", "rv_pruner_destroy")
    for name in names:
        assert name in _lib.SYMBOLS and name in _lib.ARGTYPES, name
        assert re.search(r"\b" + name + r"\s*\(", hdr), name
        assert getattr(L, name) is not None
    assert C.sizeof(_lib.PrunerInfo) == 48 and "} rv_pruner_info;" in hdr
    assert [n for n, _ in _lib.PrunerInfo._fields_] == ["total_ops", "n_kept", "state_bytes", "peak_feed_bytes", "mark_feeds", "host_feeds"]
    assert C.sizeof(_lib.PruneInfo) == 96 and L.rv_abi_version() == 8  # (calls were added, nothing changed)
    assert callable(prune.DevicePruner) and callable(prune.prune_pieces) and callable(prune.window_pieces)
    assert reverie_amd.prune_ops is prune.prune_ops


def test_windows_host_equals_whole(L, lists):
    """records, old_index and info of rv_ops_prune, for every list and cutting"""
    for (name, ops, wc, og, oz), cuts, (want_keep, _) in lists:
        rc0, want_ops, want_old, want_info = whole_host(L, ops, wc, og, oz)
        assert rc0 == 0 and want_ops.tobytes() == ops[want_keep].tobytes(), name
        for c in cuts:
            rc, out, old, info, n_out = windows_host(L, ops, wc, og, oz, c)
            assert rc == 0 and n_out == len(want_ops), (name, c)
            assert out[:n_out].tobytes() == want_ops.tobytes() and (old[:n_out] == want_old).all() and info == want_info, (name, c)
            assert (out[n_out:].view(np.uint8) == 0xA5).all()


def test_windows_host_arguments(L):
    name, ops, wc, og, oz = {c[0]: c for c in pc.corpus()}["b2a_output"]
    n = len(ops)
    for bad in ([n + 1], [5, 4], [0, n, n + 1]):
        assert windows_host(L, ops, wc, og, oz, bad)[0] == prune_ref.ARG
    kept = whole_host(L, ops, wc, og, oz)[1]
    rc, out, _, _, _ = windows_host(L, ops, wc, og, oz, [3, 3, 70], cap=len(kept) - 1)
    assert rc == prune_ref.ARG and (out.view(np.uint8) == 0xA5).all()
    assert windows_host(L, ops, wc, og, oz, [0, 0, 3, 3, n, n])[0] == 0


@pytest.mark.parametrize("case", pc.error_cases(), ids=[c[0] for c in pc.error_cases()])
def test_codes(L, case):
    name, ops, wc, og, oz, _ = case
    want = whole_host(L, ops, wc, og, oz)[0]
    assert want != 0
    n = len(ops)
    for cuts in ([], [1], [n // 2], sorted({1, n // 3, n - 1}) if n >= 3 else [0]):
        rc, out, _, _, _ = windows_host(L, ops, wc, og, oz, cuts)
        assert rc == want and (out.view(np.uint8) == 0xA5).all(), cuts


def to_file(case, cuts):
    name, ops, wc, og, oz = case[:5]
    g, z, c = np.asarray(og, np.uint32), np.asarray(oz, np.uint32), np.asarray(cuts, np.uint64)
    return struct.pack("<6Q", len(ops), wc[0], wc[1], g.size, z.size, c.size) + np.ascontiguousarray(ops).tobytes() + g.tobytes() + z.tobytes() + c.tobytes()


def test_window_step_under_sanitizers(L, lists, tmp_path):
    """the stand-alone program: clean under AddressSanitizer and UBSan; the device's order of work over prune.h's window step gives
    the host sweep's flags and needed tables window by window (the program compares), and the flags and summed layers of the Python
    model (compared here)"""
    exe = str(tmp_path / "prune_window_model")
    csrc = os.path.join(ROOT, "reverie_amd", "csrc")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", csrc,
                           "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "prune_window_model.cpp"), "-o", exe])
    jobs, paths = [], []
    for case, cuts, _ in lists:
        if len(case[1]) > 3100:
            continue
        for c in cuts[:6]:
            path = str(tmp_path / f"{len(jobs):04d}.ops")
            with open(path, "wb") as f:
                f.write(to_file(case, c))
            jobs.append((case, c))
            paths.append(path)
    assert len(jobs) > 500
    run = subprocess.run([exe] + paths, capture_output=True, text=True)
    assert run.returncode == 0 and "Sanitizer" not in run.stderr and "runtime error" not in run.stderr, (run.stdout[-2000:], run.stderr[-2000:])
    lines = run.stdout.split("\n")
    assert lines[-2] == "bad 0"
    answers = {ln.split(" ")[0]: ln.split(" ")[1:] for ln in lines if re.match(r"\d\d\d\d\.ops ", ln)}
    assert len(answers) == len(jobs)
    for k, ((name, ops, wc, og, oz), c) in enumerate(jobs):
        layers, flags = answers[f"{k:04d}.ops"]
        keep, info = pw.prune_windows(ops, c, og, oz)
        assert flags == "".join("1" if x else "0" for x in keep.tolist()), (name, c)
        assert int(layers) == info["device_rounds"], (name, c)


def test_window_pieces_on_a_host_array_and_a_memmap(tmp_path):
    from reverie_amd.prune import prune_pieces, window_pieces

    ops = pc.of_length(1000, 5)[0]
    path = str(tmp_path / "p.rvops")
    ops.tofile(path)
    for src in (ops, np.memmap(path, dtype=OP_DTYPE, mode="r", shape=(len(ops),))):
        pieces = window_pieces(src, 256)
        fwd, bwd = list(pieces()), list(pieces.backwards())
        assert [len(p) for p, _ in fwd] == [256, 256, 256, 232] and all(c is None for _, c in fwd)
        assert np.concatenate([np.asarray(p) for p, _ in fwd]).tobytes() == ops.tobytes()
        assert [np.asarray(p).tobytes() for p, _ in bwd] == [np.asarray(p).tobytes() for p, _ in fwd][::-1]
    assert list(window_pieces(ops[:0], 4)()) == []
    with pytest.raises(ValueError):
        window_pieces(ops, 0)
    # a source that cannot be read backwards is refused before anything is made, and the message names the ones that can
    with pytest.raises(TypeError) as e:
        prune_pieces(lambda: iter([(ops, None)]), (40, 70))
    for word in ("LinkPlan.pieces", "window_pieces", "backwards=", "rvops"):
        assert word in str(e.value)
    with pytest.raises(TypeError):
        prune_pieces([(ops, None)], (40, 70))


def test_command_line_refuses_other_sources(tmp_path, capsys):
    from reverie_amd.__main__ import main

    bristol = str(tmp_path / "c.txt")
    with open(bristol, "w") as f:
        f.write("1 3\n2 1 1\n1 1\n\n2 1 0 1 2 AND\n")
    base = ["--operation", "convert", "--program-path", bristol, "--output-path", str(tmp_path / "o.rvops"), "--output-format", "rvops", "--prune-windows"]
    for extra in ([], ["--program-format", "bristol", "--parser", "device", "--window-mb", "1"], ["--program-format", "mcircuit-bincode"]):
        with pytest.raises(SystemExit) as e:
            main(base + extra)
        assert e.value.code == 2
        assert "--prune-windows needs a source that can be read backwards" in capsys.readouterr().err
    prog = str(tmp_path / "p.rvops")
    program([GF2.Input(0), GF2.Mul(1, 0, 0), GF2.AssertZero(0)]).tofile(prog)
    rv = ["--operation", "convert", "--program-path", prog, "--output-path", str(tmp_path / "o.rvops"), "--output-format", "rvops", "--prune-windows"]
    for extra, word in ((["--prune"], "cannot be combined"), (["--compact-wires"], "cannot be combined")):
        with pytest.raises(SystemExit) as e:
            main(rv + extra)
        assert e.value.code == 2 and word in capsys.readouterr().err
    with pytest.raises(SystemExit) as e:
        main(["--operation", "prove", "--program-path", prog, "--witness-path", prog, "--proof-path", str(tmp_path / "x"), "--prune-windows"])
    assert e.value.code == 2 and "needs a streamed operation" in capsys.readouterr().err
