"""rv_ops_fold_windows_host, the window step's definition in C (no GPU): for every list and every cutting its records and info are
rv_ops_fold's (which tests/test_fold_host.py pins to the Python model of the sweep); the Python model of the window step
(tests/fold_window_ref.py, which shares no code with either) gives the same; the named windows of DESIGN §24.8; the codes; the
kernels' order of work on windows -- reverie_amd/csrc/fold.h run as plain CPU loops -- in a stand-alone program built with
-fsanitize=address,undefined (tests/fold_window_model.cpp); the Python face and the command line's refusal."""
import ctypes as C
import os
import re
import struct
import subprocess

import numpy as np
import pytest

import fold_cases as fc
import fold_window_ref as fw
from conftest import ROOT
from reverie_amd.ops import B2A, GF2, OP_DTYPE, Z64, program


@pytest.fixture(scope="module")
def L():
    from reverie_amd import _lib

    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__

        __graft_entry__.build()
    return _lib.lib()


@pytest.fixture(scope="module")
def corpus(L):
    lim = (C.c_uint32 * 5)()
    assert L.rv_hook_fold_limits(lim) == 0
    return fc.corpus(int(lim[1]))


@pytest.fixture(scope="module")
def generated():
    return fc.generated()


_whole = {}


def _p(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None and a.size else None


def _dict(fi):
    return {k: int(getattr(fi, k)) for k, _ in fi._fields_}


def whole(L, case):
    """rv_ops_fold's (records, info) of a case, computed once"""
    from reverie_amd import _lib

    name, ops, wc = case[:3]
    if name not in _whole:
        ops = np.ascontiguousarray(ops)
        out, fi = np.empty_like(ops), _lib.FoldInfo()
        assert L.rv_ops_fold(_p(ops), len(ops), int(wc[0]), int(wc[1]), _p(out), C.byref(fi)) == 0
        _whole[name] = (out, _dict(fi))
    return _whole[name]


def host_windows(L, ops, wc, cuts, out="new"):
    """rv_ops_fold_windows_host through ctypes -> (code, records or None, info dict); out: "new", "inplace", None"""
    from reverie_amd import _lib

    ops = np.ascontiguousarray(ops)
    n = len(ops)
    fi = _lib.FoldInfo()
    c = np.asarray(cuts, dtype=np.uintp)
    # (room for one record more: the record behind the list must stay)
    buf = ops.copy() if out == "inplace" else np.full((n + 1) * 24, 0xEE, np.uint8).view(OP_DTYPE) if out == "new" else None
    src = buf if out == "inplace" else ops
    rc = L.rv_ops_fold_windows_host(_p(src), n, int(wc[0]), int(wc[1]), _p(c), len(c), _p(buf) if out and n else None, C.byref(fi))
    if out == "new":
        assert (buf[n:].view(np.uint8) == 0xEE).all()
        buf = buf[:n]
    return rc, buf, _dict(fi)


def check_cutting(L, case, cuts, label=""):
    want, winfo = whole(L, case)
    rc, got, info = host_windows(L, case[1], case[2], cuts)
    assert rc == 0 and got.tobytes() == want.tobytes() and info == winfo, (case[0], label, cuts)


def test_symbols_exported_and_bound(L):
    from reverie_amd import _lib, fold

    hdr = open(os.path.join(ROOT, "include", "reverie_amd.h")).read()
    for name in ("rv_ops_fold_windows_host", "rv_folder_begin", "rv_folder_feed", "rv_folder_end", "rv_folder_rewind", "rv_folder_replay",
                 "rv_folder_replay_end", "rv_folder_get_info", "rv_folder_destroy"):
        assert name in _lib.SYMBOLS and name in _lib.ARGTYPES and getattr(L, name) is not None
        assert re.search(r"\b" + name + r"\s*\(", hdr), name
    assert C.sizeof(_lib.FolderInfo) == 56 and re.search(r"#define RV_FOLDER_KEEP_LOG 1u", hdr) and fold.KEEP_LOG == 1
    assert [n for n, _ in _lib.FolderInfo._fields_] == ["total_ops", "state_bytes", "log_bytes", "log_records", "peak_feed_bytes", "feeds", "host_feeds"]
    assert L.rv_abi_version() == 8  # (calls were added, nothing changed)
    for name in ("DeviceFolder", "fold_pieces", "fold_windows_host"):
        assert callable(getattr(fold, name))


def test_host_equals_whole_on_corpus(L, corpus):
    """every case, every cutting of fold_window_ref.cuttings: the records and the info of the whole-list call"""
    for k, case in enumerate(corpus):
        rng = np.random.default_rng(4000 + k)
        for label, cuts in fw.cuttings(len(case[1]), rng):
            check_cutting(L, case, cuts, label)


def test_host_equals_whole_on_generated_lists(L, generated):
    assert len(generated) == 400
    for k, case in enumerate(generated):
        rng = np.random.default_rng(5000 + k)
        for label, cuts in fw.cuttings(len(case[1]), rng):
            check_cutting(L, case, cuts, label)


def test_window_model_equals_whole(L, corpus, generated):
    """the Python model of the window step -- resolve, seed, layers, rewrite, last-writer update, on dicts -- reaches rv_ops_fold's
    records and counts, and rv_ops_fold_windows_host's in place, on the same cuttings (lists of at most 700 ops, and every fourth
    generated list); its log replays to the folded list window by window; a single window's layer count is the sweep model's"""
    import fold_ref

    cases = [c for c in corpus if len(c[1]) <= 700] + generated[::4]
    for k, case in enumerate(cases):
        want, winfo = whole(L, case)
        rng = np.random.default_rng(6000 + k)
        for label, cuts in fw.cuttings(len(case[1]), rng, every_single=24):
            rc, got, info, layers, log = fw.fold_windows(case[1], case[2], cuts)
            assert rc == 0 and got.tobytes() == want.tobytes(), (case[0], label, cuts)
            hrc, hgot, hinfo = host_windows(L, case[1], case[2], cuts, out="inplace")
            assert hrc == 0 and hgot.tobytes() == got.tobytes() and {k2: hinfo[k2] for k2 in info} == info, (case[0], label, cuts)
            assert info == {k2: v for k2, v in winfo.items() if k2 in info}, (case[0], label)
            assert len(log) == winfo["n_rewritten"] and [o for o, _ in log] == sorted(o for o, _ in log)
            if label == "whole":
                assert layers == [len(fold_ref.layers(case[1])[1])], case[0]
                for first in range(0, len(want), 97):
                    assert fw.replay(case[1], log, first, 97).tobytes() == want[first:first + 97].tobytes()


# ---- the named windows ----
def named_windows(corpus):
    """(name, ops, wire counts, cuts, what the cutting is for)"""
    cases = {c[0]: c for c in corpus}
    out = [("const_and_reader", program([GF2.Input(0), GF2.Const(1, 1), GF2.Mul(2, 0, 1), GF2.Add(3, 1, 1)]), (0, 4), [2],
            "a Const and its readers on either side of the cut")]
    # known_then_unknown: index 1 is Const 1 (op 1), Add of Inputs (op 3), Const 0 (op 5), Input (op 7); its readers are ops 2, 4, 6, 8
    out.append(("known_then_unknown",) + cases["known_then_unknown"][1:] + ([2, 4, 6, 8, 11, 13], "cut between each redefinition and its next reader"))
    # unknown_then_known: index 1 is Input (op 1), Const 9 (op 3), Mul (op 5); index 0 is Input (op 0), Sub (op 7); GF(2) 0: ops 9, 10, 11
    out.append(("unknown_then_known",) + cases["unknown_then_known"][1:] + ([2, 4, 6, 8, 10, 11, 12], "cut between each redefinition and its next reader"))
    out.append(("never_written_third_window", program([Z64.Input(0), Z64.Input(1), Z64.Mul(2, 0, 1), Z64.Add(3, 0, 7), Z64.Mul(4, 7, 1), Z64.AssertZero(7),
                                                       Z64.AddConst(5, 7, 3)]), (8, 0), [1, 3], "index 7 is never written and read in the third window"))
    # sizehint_grows: SizeHints at ops 1, 4, 5
    out.append(("sizehint_grows",) + cases["sizehint_grows"][1:] + ([2, 5, 6], "cut straight after each SizeHint: a new index is known 0 from a grown table"))
    for name, ops, wc in fc.b2a_cases():
        b2a = int(np.flatnonzero(ops["domain"] == 2)[0])
        out.append((name + "_alone_in_third", ops, wc, [b2a // 2, b2a, b2a + 1], "the 64 bits are written in two earlier windows, the B2A stands alone"))
    chain = cases["known_chain_65"]
    out.append(("known_chain_65_middle",) + chain[1:] + ([len(chain[1]) // 2], "the chain is cut in its middle"))
    out.append(("mul_zero_escapes", program([GF2.Const(0, 0), Z64.Const(0, 0), GF2.Input(1), GF2.Mul(2, 0, 1), GF2.Mul(3, 1, 0), Z64.Input(1), Z64.Mul(2, 1, 0),
                                             Z64.Add(3, 1, 0)]), (4, 4), [2], "a Mul whose known-0 operand escapes while the other is an in-window Input"))
    return out


def test_named_windows(L, corpus):
    for name, ops, wc, cuts, why in named_windows(corpus):
        case = ("named_" + name, ops, wc)
        want, winfo = whole(L, case)
        rc, got, info = host_windows(L, ops, wc, cuts)
        assert rc == 0 and got.tobytes() == want.tobytes() and info == winfo, (name, why)
        rc, got, info, _, log = fw.fold_windows(ops, wc, cuts)
        assert rc == 0 and got.tobytes() == want.tobytes() and len(log) == winfo["n_rewritten"], (name, why)
    # what the named windows are about, said in records
    named = {c[0]: c for c in named_windows(corpus)}
    _, ops, wc, cuts, _ = named["const_and_reader"]
    got = host_windows(L, ops, wc, cuts)[1]
    assert got[2].tolist() == (0, 7, 0, 2, 0, 0, 1) and got[3].tolist() == (0, 9, 0, 3, 0, 0, 0)  # MulConst by the carried 1; Const 1 ^ 1
    _, ops, wc, cuts, _ = named["never_written_third_window"]
    got, info = host_windows(L, ops, wc, cuts)[1:]
    assert got[3].tolist() == (1, 3, 0, 3, 0, 0, 0) and got[4].tolist() == (1, 9, 0, 4, 0, 0, 0) and got[6].tolist() == (1, 9, 0, 5, 0, 0, 3)
    assert info["asserts_known_zero"] == 1
    _, ops, wc, cuts, _ = named["mul_zero_escapes"]
    got = host_windows(L, ops, wc, cuts)[1]
    assert [r.tolist() for r in got[[3, 4, 6]]] == [(0, 9, 0, 2, 0, 0, 0), (0, 9, 0, 3, 0, 0, 0), (1, 9, 0, 2, 0, 0, 0)]
    assert got[7].tolist() == (1, 3, 0, 3, 1, 0, 0)  # Add with the carried 0: AddConst 0
    _, ops, wc, cuts, _ = named["b2a_64_known_alone_in_third"]
    got = host_windows(L, ops, wc, cuts)[1]
    assert got[cuts[1]]["domain"] == 1 and got[cuts[1]]["opcode"] == 9


# ---- errors ----
@pytest.mark.parametrize("case", fc.error_cases(), ids=[c[0] for c in fc.error_cases()])
def test_codes(L, case):
    """rv_ops_fold's code whatever the cuts; nothing is written; the window model names the same code"""
    name, ops, wc = case
    want = L.rv_ops_fold(_p(ops), len(ops), wc[0], wc[1], None, None)
    assert want != 0
    for cuts in ([], [len(ops) // 2], list(range(1, len(ops), 7))):
        rc, out, _ = host_windows(L, ops, wc, cuts)
        assert rc == want and (out.view(np.uint8) == 0xEE).all(), (name, cuts)
        assert host_windows(L, ops, wc, cuts, out=None)[0] == want
        assert host_windows(L, ops, wc, cuts, out="inplace")[1].tobytes() == ops.tobytes()
        assert fw.fold_windows(ops, wc, cuts)[0] == want


def test_bad_cuts_and_overlap(L, corpus):
    case = {c[0]: c for c in corpus}["length_257"]
    name, ops, wc = case
    n = len(ops)
    want, winfo = whole(L, case)
    for cuts in ([n + 1], [5, 4], [0, n, n - 1], [1 << 40]):
        rc, out, _ = host_windows(L, ops, wc, cuts)
        assert rc == fw.ARG and (out.view(np.uint8) == 0xEE).all(), cuts
    p = np.ascontiguousarray(ops)
    assert L.rv_ops_fold_windows_host(_p(p), n, wc[0], wc[1], None, 1, None, None) == fw.ARG  # cuts announced, none given
    assert L.rv_ops_fold_windows_host(None, n, wc[0], wc[1], None, 0, None, None) == fw.ARG
    assert L.rv_ops_fold_windows_host(None, 0, 0, 0, None, 0, None, None) == 0
    # in place
    rc, got, info = host_windows(L, ops, wc, [3, 100, 256], out="inplace")
    assert rc == 0 and got.tobytes() == want.tobytes() and info == winfo
    assert host_windows(L, ops, wc, [3, 100, 256], out=None)[2] == winfo
    # any other overlap
    both = np.concatenate([p, p])
    cuts = np.asarray([100], dtype=np.uintp)
    for off in (24, 24 * (n - 1)):
        assert L.rv_ops_fold_windows_host(_p(both), n, wc[0], wc[1], _p(cuts), 1, C.c_void_p(both.ctypes.data + off), None) == fw.ARG
    assert L.rv_ops_fold_windows_host(C.c_void_p(both.ctypes.data + 24), n - 1, wc[0], wc[1], _p(cuts), 1, _p(both), None) == fw.ARG
    assert both.tobytes() == np.concatenate([p, p]).tobytes()


# ---- the kernels' order of work on windows, under the sanitizers ----
def to_file(case, cuts):
    name, ops, wc = case[:3]
    return struct.pack("<4Q", len(ops), wc[0], wc[1], len(cuts)) + struct.pack("<%dQ" % len(cuts), *cuts) + np.ascontiguousarray(ops).tobytes()


def fnv(data: bytes) -> int:
    h = 1469598103934665603
    for b in data:
        h = ((h ^ b) * 1099511628211) & 0xFFFFFFFFFFFFFFFF
    return h


def test_window_model_under_sanitizers(L, corpus, generated, tmp_path):
    """the stand-alone program: clean under AddressSanitizer and UBSan; for every case and cutting the kernels' order of work --
    escape lookup, seed, pairs, layers, log append, rewrite, last-writer table update, table growth, and a replay of the log over
    windows cut differently -- gives rv_ops_fold_windows_host's code, records, info and log length (the program compares); the bytes
    are rv_ops_fold's (compared here, by digest), and a single window's layers are the sweep model's"""
    import fold_ref

    exe = str(tmp_path / "fold_window_model")
    csrc = os.path.join(ROOT, "reverie_amd", "csrc")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", csrc,
                           os.path.join(ROOT, "tests", "fold_window_model.cpp"), os.path.join(csrc, "fold.cpp"), "-o", exe])
    runs = []
    named = [(("named_" + n, o, w), cuts) for n, o, w, cuts, _ in named_windows(corpus)]
    for k, case in enumerate(list(corpus) + generated[:40]):
        rng = np.random.default_rng(7000 + k)
        for label, cuts in fw.cuttings(len(case[1]), rng):
            runs.append((case, cuts, 0))
    runs += [(c, cuts, 0) for c, cuts in named]
    runs += [(c, cuts, fold_ref.check(c[1], c[2])) for c in fc.error_cases() for cuts in ([], [len(c[1]) // 3, len(c[1]) // 2])]
    paths = []
    for k, (case, cuts, _) in enumerate(runs):
        path = str(tmp_path / f"{k:04d}.ops")
        with open(path, "wb") as f:
            f.write(to_file(case, cuts))
        paths.append(path)
    listing = str(tmp_path / "files.txt")
    with open(listing, "w") as f:
        f.write("\n".join(paths) + "\n")
    run = subprocess.run([exe, "@" + listing], capture_output=True, text=True)
    assert run.returncode == 0 and "Sanitizer" not in run.stderr and "runtime error" not in run.stderr, (run.stdout[-2000:], run.stderr[-2000:])
    lines = run.stdout.split("\n")
    assert lines[-2] == "bad 0"
    answers = {ln.split()[0]: ln.split()[1:] for ln in lines if re.match(r"\d\d\d\d\.ops", ln)}
    assert len(answers) == len(runs)
    for k, (case, cuts, code) in enumerate(runs):
        rc, n_known, layers, n_log, digest = answers[f"{k:04d}.ops"]
        assert int(rc) == code, case[0]
        if code:
            continue
        want, winfo = whole(L, case)
        assert int(n_known) == winfo["n_known"] and int(n_log) == winfo["n_rewritten"] and int(digest, 16) == fnv(want.tobytes()), (case[0], cuts)
        if not cuts:
            assert int(layers) == len(fold_ref.layers(case[1])[1]), case[0]
    # the bound: cut in three, the depth-65 chain's windows stop after 3 layers and are stepped by the host sweep, with the same bytes
    chain = {c[0]: c for c in corpus}["known_chain_65"]
    path = str(tmp_path / "chain.ops")
    with open(path, "wb") as f:
        f.write(to_file(chain, [2, 40]))
    run = subprocess.run([exe, "--max-rounds", "3", path], capture_output=True, text=True)
    assert run.returncode == 0 and "Sanitizer" not in run.stderr, run.stderr[-2000:]
    first = run.stdout.split("\n")[0].split()
    assert first[1] == "0" and int(first[5], 16) == fnv(whole(L, chain)[0].tobytes()) and first[6:] == ["fallback", "2"]


# ---- the Python face ----
def test_python_face(L, corpus):
    from reverie_amd import ReverieError, fold

    case = {c[0]: c for c in corpus}["length_513"]
    name, ops, wc = case
    want, winfo = whole(L, case)
    for cuts in ((), [100], np.asarray([0, 256, 256, 513])):
        out, info = fold.fold_windows_host(ops, wc, cuts)
        assert out.tobytes() == want.tobytes() and info == winfo and out.dtype == OP_DTYPE
    out, info = fold.fold_windows_host([GF2.Const(0, 1), GF2.Input(1), GF2.Mul(2, 0, 1)], cuts=[1])
    assert out[2].tolist() == (0, 7, 0, 2, 1, 0, 1) and info["gf2_mul_to_linear"] == 1
    assert fold.fold_windows_host([], cuts=[0])[1]["n_ops"] == 0
    with pytest.raises(ReverieError) as e:
        fold.fold_windows_host(ops, wc, [514])
    assert e.value.code == fw.ARG
    with pytest.raises(ValueError):
        fold.fold_windows_host(ops, wc, [-1])
    with pytest.raises(TypeError):
        fold.fold_pieces(iter([]), wc)


def test_refusal_points_at_fold_pieces(L):
    from reverie_amd import stream

    pieces = lambda: iter([(program([Z64.Input(0)]), None)])
    for fn, args in ((stream.prove_streaming_pieces, (pieces, [], [5], (1, 0))), (stream.verify_streaming_pieces, (pieces, (1, 0), b"")),
                     (stream.evaluate_streaming_pieces, (pieces, [], [5], (1, 0)))):
        with pytest.raises(ValueError) as e:
            fn(*args, fold=True)
        assert "a window's unwritten index is not the list's" in str(e.value) and "fold.fold_pieces" in str(e.value)


def test_command_line_refusals(L, tmp_path, capsys):
    from reverie_amd.__main__ import main

    prog = str(tmp_path / "p.rvops")
    program([GF2.Input(0), GF2.Const(1, 1), GF2.Mul(2, 0, 1), GF2.AssertZero(2)]).tofile(prog)
    bristol = str(tmp_path / "p.txt")
    open(bristol, "w").write("1 3\n2 1 1\n1 1\n\n2 1 0 1 2 AND\n")
    wit = str(tmp_path / "w.txt")
    open(wit, "w").write("10")
    # a source that is read whole: the resident prover, a Bristol file on the host parser, a device parser without windows
    whole_sources = (["--operation", "prove", "--program-path", prog, "--witness-path", wit, "--proof-path", str(tmp_path / "x")],
                     ["--operation", "prove", "--stream", "--program-path", bristol, "--witness-path", wit, "--proof-path", str(tmp_path / "x")],
                     ["--operation", "oneshot", "--evaluator", "stream", "--parser", "device", "--program-path", bristol, "--witness-path", wit],
                     ["--operation", "convert", "--program-path", bristol, "--output-path", str(tmp_path / "o"), "--output-format", "rvops"],
                     # (convert reads a bincode file in windows only with --window-mb, --stream or not)
                     ["--operation", "convert", "--stream", "--parser", "device", "--program-format", "mcircuit-bincode", "--program-path", bristol,
                      "--output-path", str(tmp_path / "o"), "--output-format", "rvops"])
    for args in whole_sources:
        with pytest.raises(SystemExit) as e:
            main(args + ["--fold-windows"])
        assert e.value.code == 2
        err = capsys.readouterr().err
        assert "--fold-windows needs a source that is read in windows" in err and "folded by --fold" in err
    # and the whole-list flags are not its partners
    for extra in (["--fold"], ["--prune"], ["--compact-wires"]):
        with pytest.raises(SystemExit) as e:
            main(["--operation", "convert", "--program-path", prog, "--output-path", str(tmp_path / "o"), "--output-format", "rvops", "--fold-windows"] + extra)
        assert e.value.code == 2
        assert "--fold-windows" in capsys.readouterr().err
