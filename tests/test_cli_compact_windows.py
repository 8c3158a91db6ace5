"""`python -m reverie_amd --compact-windows`: a Bristol file read in windows on the GPU, compacted in windows and proved / verified as
a stream -- the proof and the stderr line are --compact-wires' (the command line draws its seeds from the OS: the tests put fixed
ones in their place); the flag without a windowed source is an argparse error."""
import pytest

from reverie_amd.__main__ import build_parser, main
from test_cli_compact import adder_files


def test_flag_needs_a_windowed_source(tmp_path, capsys):
    assert build_parser().parse_args(["--operation", "prove", "--compact-windows"]).compact_windows
    assert not build_parser().parse_args(["--operation", "prove"]).compact_windows
    p, w, e = adder_files(tmp_path)
    common = ["--program-path", str(p), "--expected-outputs-path", str(e), "--witness-path", str(w), "--proof-path", str(tmp_path / "x.bin")]
    for args in (["--operation", "prove"],  # not streamed
                 ["--operation", "prove", "--stream"],  # the host parser reads the file whole
                 ["--operation", "prove", "--stream", "--parser", "device"],  # a Bristol file without --window-mb is parsed whole
                 ["--operation", "prove", "--parser", "device", "--window-mb", "1"],
                 ["--operation", "oneshot", "--evaluator", "gpu", "--parser", "device", "--window-mb", "1"],
                 ["--operation", "prove", "--stream", "--parser", "device", "--window-mb", "1", "--compact-wires"]):
        with pytest.raises(SystemExit) as x:
            main(args + ["--compact-windows"] + common)
        assert x.value.code == 2 and "--compact-windows" in capsys.readouterr().err


@pytest.mark.gpu
def test_cli_compact_windows_roundtrip(tmp_path, capsys, monkeypatch, rule_seeds):
    from reverie_amd import stream

    p, w, e = adder_files(tmp_path)
    plain = stream.prove_streaming_pieces
    monkeypatch.setattr(stream, "prove_streaming_pieces", lambda *a, **k: plain(*a, **{**k, "seeds": rule_seeds}))
    common = ["--program-path", str(p), "--expected-outputs-path", str(e), "--stream", "--parser", "device", "--window-mb", "1"]
    whole, windows = tmp_path / "proof_whole.bin", tmp_path / "proof_windows.bin"
    assert main(["--operation", "prove", "--witness-path", str(w), "--proof-path", str(whole), "--compact-wires"] + common) == 0
    line = [x for x in capsys.readouterr().err.splitlines() if x.startswith("compact-wires: wire counts")]
    assert len(line) == 1
    assert main(["--operation", "prove", "--witness-path", str(w), "--proof-path", str(windows), "--compact-windows"] + common) == 0
    assert [x for x in capsys.readouterr().err.splitlines() if x.startswith("compact-wires:")] == line
    assert windows.read_bytes() == whole.read_bytes()
    for flag in ("--compact-windows", "--compact-wires"):
        assert main(["--operation", "verify", "--proof-path", str(windows), flag] + common) == 0
    assert [x for x in capsys.readouterr().err.splitlines() if x.startswith("compact-wires:")] == line * 2
    # oneshot-zk proves and verifies from the same compacted pieces (three passes over one compactor)
    assert main(["--operation", "oneshot-zk", "--witness-path", str(w), "--compact-windows"] + common) == 0
    out = capsys.readouterr()
    assert out.out.count("Ok(())") == 1 and [x for x in out.err.splitlines() if x.startswith("compact-wires:")] == line
    assert main(["--operation", "oneshot", "--evaluator", "stream", "--witness-path", str(w), "--compact-windows"] + common[:4] + common[5:]) == 0
    assert line[0] in capsys.readouterr().err
    bad = bytearray(windows.read_bytes())
    bad[len(bad) // 2] ^= 1
    (tmp_path / "bad.bin").write_bytes(bytes(bad))
    try:
        assert main(["--operation", "verify", "--proof-path", str(tmp_path / "bad.bin"), "--compact-windows"] + common) == 1
    except Exception as x:  # (a proof the library cannot parse is refused with an error)
        assert type(x).__name__ == "ReverieError"
