"""`python -m reverie_amd --operation convert` with --parser host (no GPU): a Bristol file to rvops, to mcircuit-bincode and back to
Bristol text with the records intact; --compact-wires; what Bristol output refuses; the arguments that belong to convert alone."""
import os
import subprocess
import sys

import numpy as np
import pytest

import bristol_gen
from conftest import ROOT
from reverie_amd.ops import OP_DTYPE, Z64, program


def cli(*args):
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    return subprocess.run([sys.executable, "-m", "reverie_amd", *args], capture_output=True, text=True, env=env, cwd=ROOT)


@pytest.fixture(scope="module")
def lib():
    from reverie_amd import _lib

    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__

        __graft_entry__.build()
    return _lib.lib()


@pytest.fixture(scope="module")
def source(tmp_path_factory, lib):
    from reverie_amd import bristol

    d = tmp_path_factory.mktemp("convert")
    text = bristol_gen.adder64()
    path = str(d / "adder64.txt")
    open(path, "w").write(text)
    prog, info = bristol.parse(text)
    return d, path, prog, info


def test_bristol_to_rvops_to_bincode_and_back(source):
    from reverie_amd import bristol, program_file

    d, path, prog, info = source
    rvops, binc, back = str(d / "a.rvops"), str(d / "a.bin"), str(d / "back.txt")
    r = cli("--operation", "convert", "--program-path", path, "--output-path", rvops, "--output-format", "rvops")
    assert r.returncode == 0, r.stderr
    assert np.fromfile(rvops, OP_DTYPE).tobytes() == prog.tobytes()
    wc = info["wire_counts"]
    assert r.stderr.strip().endswith("convert: %d ops, wire counts (z64, gf2) %s -> %s, %d bytes" % (len(prog), wc, wc, 24 * len(prog)))
    r = cli("--operation", "convert", "--program-path", rvops, "--output-path", binc, "--output-format", "mcircuit-bincode")
    assert r.returncode == 0, r.stderr
    assert open(binc, "rb").read() == program_file.dumps(prog)
    r = cli("--operation", "convert", "--program-path", binc, "--program-format", "mcircuit-bincode", "--output-path", back, "--output-format", "bristol")
    assert r.returncode == 0, r.stderr
    again, info2 = bristol.parse(open(back, "rb").read())
    assert again.tobytes() == prog.tobytes() and info2["n_wires"] == info["n_wires"] and info2["n_inputs"] == info["n_inputs"]
    # straight from the text the header keeps its output count too
    r = cli("--operation", "convert", "--program-path", path, "--output-path", back, "--output-format", "bristol")
    assert r.returncode == 0, r.stderr
    again, info2 = bristol.parse(open(back, "rb").read())
    assert again.tobytes() == prog.tobytes() and info2["n_outputs"] == info["n_outputs"] == 64
    assert open(back, "rb").read() == bristol.dumps(prog, 64)


def test_compact_wires(source):
    from reverie_amd.compact import compact_wires

    d, path, prog, info = source
    out = str(d / "compact.rvops")
    r = cli("--operation", "convert", "--program-path", path, "--compact-wires", "--output-path", out, "--output-format", "rvops")
    assert r.returncode == 0, r.stderr
    want, wc, _ = compact_wires(prog, info["wire_counts"])
    assert np.fromfile(out, OP_DTYPE).tobytes() == want.tobytes() and wc[1] < info["wire_counts"][1]
    assert "convert: %d ops, wire counts (z64, gf2) %s -> %s, %d bytes" % (len(prog), info["wire_counts"], wc, 24 * len(prog)) in r.stderr
    # ... and as Bristol text: the compacted count in the header, no outputs
    txt = str(d / "compact.txt")
    r = cli("--operation", "convert", "--program-path", path, "--compact-wires", "--output-path", txt, "--output-format", "bristol")
    assert r.returncode == 0, r.stderr
    assert open(txt, "rb").read().split(b"\n")[:3] == [b"%d %d" % (len(prog) - 128, wc[1]), b"1 128", b"1 0"]


def test_bristol_output_refuses_what_it_cannot_say(source):
    d, path, prog, info = source
    exp = str(d / "expected.txt")
    open(exp, "w").write("0" * 64)
    out = str(d / "refused.txt")
    r = cli("--operation", "convert", "--program-path", path, "--expected-outputs-path", exp, "--output-path", out, "--output-format", "bristol")
    assert r.returncode != 0 and "--expected-outputs-path" in r.stderr
    # the same source converts to a program file, assertions and all
    r = cli("--operation", "convert", "--program-path", path, "--expected-outputs-path", exp, "--output-path", out, "--output-format", "mcircuit-bincode")
    assert r.returncode == 0 and "convert: %d ops" % (len(prog) + 128) in r.stderr
    z = str(d / "z64.rvops")
    program([Z64.Input(0), Z64.Input(1), Z64.Add(2, 0, 1)]).tofile(z)
    r = cli("--operation", "convert", "--program-path", z, "--output-path", out, "--output-format", "bristol")
    assert r.returncode != 0 and "cannot be written as Bristol text (op 0)" in r.stderr
    mixed = str(d / "mixed.rvops")
    q = prog.copy()
    q["opcode"][200] = 4  # Sub
    q.tofile(mixed)
    r = cli("--operation", "convert", "--program-path", mixed, "--output-path", out, "--output-format", "bristol")
    assert r.returncode != 0 and "(op 200)" in r.stderr


def test_arguments(source):
    d, path, prog, info = source
    out = str(d / "never.bin")
    r = cli("--operation", "oneshot", "--program-path", path, "--witness-path", path, "--output-path", out)
    assert r.returncode == 2 and "--operation convert" in r.stderr
    r = cli("--operation", "version_info", "--output-format", "rvops")
    assert r.returncode == 2
    r = cli("--operation", "convert", "--program-path", path, "--output-path", out)
    assert r.returncode == 2 and "--output-format is required" in r.stderr
    r = cli("--operation", "convert", "--program-path", path, "--output-format", "rvops")
    assert r.returncode == 2 and "--output-path is required" in r.stderr
    r = cli("--operation", "convert", "--program-path", path, "--output-path", out, "--output-format", "rvops", "--compact-windows", "--compact-wires")
    assert r.returncode == 2
    assert not os.path.exists(out)
