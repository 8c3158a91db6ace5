"""`python -m reverie_amd --operation convert` on the GPU: a Bristol text read in windows, compacted in windows and written as a program
file through the windowed writer; a text of several windows written back as Bristol text; a whole device parse through the whole-list
device writers; and the message for a program Bristol text cannot hold."""
import os
import subprocess
import sys

import numpy as np
import pytest

import bristol_gen
from conftest import ROOT
from reverie_amd.ops import Z64, program

pytestmark = pytest.mark.gpu


def cli(*args):
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    return subprocess.run([sys.executable, "-m", "reverie_amd", *args], capture_output=True, text=True, env=env, cwd=ROOT)


def ssa_circuit(n_in, n_gates, seed):
    """a generated SSA Bristol text (a wire per gate) and the outputs it maps `witness` to"""
    rng = np.random.default_rng(seed)
    nl = bristol_gen.Netlist(n_in)
    for _ in range(n_gates):
        a, b = int(rng.integers(max(0, nl.n - 200), nl.n)), int(rng.integers(max(0, nl.n - 40), nl.n))
        k = int(rng.integers(0, 4))
        nl.xor(a, b) if k == 0 else nl.and_(a, b) if k == 1 else nl.inv(b) if k == 2 else nl.xor(b, a)
    return nl.finish(list(range(nl.n - 16, nl.n)), [n_in], [16])


def test_windowed_compacted_program_file(tmp_path):
    from reverie_amd import bristol, compact, program_file

    text = ssa_circuit(32, 3000, 5)
    prog, _ = bristol.parse(text)
    witness = [(7 * i + 3) % 2 for i in range(32)]
    values = bristol_gen.evaluate(prog, witness)
    expected = values[len(values) - 16:]
    src, exp, out = str(tmp_path / "ssa.txt"), str(tmp_path / "expected.txt"), str(tmp_path / "ssa.bin")
    open(src, "w").write(text)
    open(exp, "w").write("".join(map(str, expected)))
    r = cli("--operation", "convert", "--program-path", src, "--expected-outputs-path", exp, "--parser", "device", "--window-mb", "1",
            "--compact-windows", "--output-path", out, "--output-format", "mcircuit-bincode")
    assert r.returncode == 0, r.stderr
    # the same source through compact_pieces
    wc = bristol.wire_counts(src, expected)
    new_wc, pieces, _ = compact.compact_pieces(lambda: bristol.iter_device(src, 1 << 20, expected), wc)
    want = b"".join(ops.cpu().numpy().tobytes() for ops, _ in pieces())
    data = open(out, "rb").read()
    got = program_file.loads(data)
    assert got.tobytes() == want and len(got) == 32 + 3016 + 32
    assert "compact-wires: wire counts (z64, gf2) %s -> %s" % (wc, new_wc) in r.stderr
    assert r.stderr.strip().endswith("convert: %d ops, wire counts (z64, gf2) %s -> %s, %d bytes" % (len(got), wc, new_wc, len(data)))
    assert new_wc[1] < wc[1] // 4  # (operands lie at most 200 wires back: few values are alive at once)
    # the converted file states the same thing: the witness satisfies it
    full, _ = bristol.parse(text, expected)
    assert len(full) == len(got)
    import reverie_amd

    assert reverie_amd.Circuit(got, new_wc).evaluate(witness, []).ok
    witness[0] ^= 1
    assert reverie_amd.Circuit(full, wc).evaluate(witness, []).ok == reverie_amd.Circuit(got, new_wc).evaluate(witness, []).ok


def test_several_windows_back_to_bristol_text(tmp_path):
    from reverie_amd import bristol

    text = bristol_gen.sha256_block()
    assert len(text) > 2 << 20  # three windows of 1 MiB
    prog, info = bristol.parse(text)
    src, out = str(tmp_path / "sha256.txt"), str(tmp_path / "back.txt")
    open(src, "w").write(text)
    r = cli("--operation", "convert", "--program-path", src, "--parser", "device", "--window-mb", "1", "--output-path", out, "--output-format", "bristol")
    assert r.returncode == 0, r.stderr
    data = open(out, "rb").read()
    assert data == bristol.dumps(prog, 256)
    wc = info["wire_counts"]
    assert r.stderr.strip().endswith("convert: %d ops, wire counts (z64, gf2) %s -> %s, %d bytes" % (len(prog), wc, wc, len(data)))


def test_whole_device_parse_and_the_refusal(tmp_path):
    from reverie_amd import bristol, program_file

    text = bristol_gen.adder64()
    prog, info = bristol.parse(text)
    src, out = str(tmp_path / "adder.txt"), str(tmp_path / "adder.bin")
    open(src, "w").write(text)
    r = cli("--operation", "convert", "--program-path", src, "--parser", "device", "--compact-wires", "--output-path", out, "--output-format", "bristol")
    assert r.returncode == 0, r.stderr
    from reverie_amd.compact import compact_wires

    want, wc, _ = compact_wires(prog, info["wire_counts"])
    assert open(out, "rb").read() == bristol.dumps_host(want, 0, wc[1])
    # a program file with a Z64 op, parsed on the GPU: the message names the op
    mixed = np.concatenate([prog, program([Z64.Input(0)])])
    open(out, "wb").write(program_file.dumps(mixed))
    r = cli("--operation", "convert", "--program-path", out, "--program-format", "mcircuit-bincode", "--parser", "device", "--output-path",
            str(tmp_path / "never.txt"), "--output-format", "bristol")
    assert r.returncode != 0 and "op %d cannot be written as Bristol text" % len(prog) in r.stderr, r.stderr
