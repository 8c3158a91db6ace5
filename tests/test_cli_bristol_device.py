"""`python -m reverie_amd --parser device`: a Bristol file parsed on the GPU gives the proof file the host parser's program gives
(the command line draws its seeds from the OS: the test puts fixed ones in their place), and each parser verifies the other's proof."""
import pytest

import bristol_gen
from reverie_amd.__main__ import build_parser, main


def adder_files(tmp_path, a=0x0123456789ABCDEF, b=0xFEDCBA9876543210):
    p = tmp_path / "adder.txt"
    p.write_text(bristol_gen.adder64())
    w = tmp_path / "wit.txt"
    w.write_text(" ".join(str((a >> i) & 1) for i in range(64)) + "\n" + " ".join(str((b >> i) & 1) for i in range(64)))
    e = tmp_path / "exp.txt"
    e.write_text("".join(str((((a + b) & (2**64 - 1)) >> i) & 1) for i in range(64)))
    return p, w, e


def test_flag(tmp_path):
    assert build_parser().parse_args(["--operation", "prove"]).parser == "host"
    assert build_parser().parse_args(["--operation", "prove", "--parser", "device"]).parser == "device"
    p, w, e = adder_files(tmp_path)
    with pytest.raises(SystemExit):  # (the host evaluator cannot read a program that lies in GPU memory)
        main(["--operation", "oneshot", "--parser", "device", "--evaluator", "host", "--program-path", str(p), "--witness-path", str(w)])


@pytest.mark.gpu
def test_cli_device_parser_roundtrip(tmp_path, capsys, monkeypatch, rule_seeds):
    from reverie_amd.proof import Proof

    p, w, e = adder_files(tmp_path)
    plain_new = Proof.new
    monkeypatch.setattr(Proof, "new", staticmethod(lambda circuit, wit_gf2, wit_z64, *a, **k: plain_new(circuit, wit_gf2, wit_z64, *a, **{**k, "seeds": rule_seeds})))
    common = ["--program-path", str(p), "--expected-outputs-path", str(e)]
    host = tmp_path / "proof_host.bin"
    assert main(["--operation", "prove", "--witness-path", str(w), "--proof-path", str(host)] + common) == 0
    for k, extra in enumerate((["--parser", "device"], ["--parser", "device", "--compiler", "device"],
                               ["--parser", "device", "--compiler", "device", "--compact-wires"])):
        dev = tmp_path / ("proof_device%d.bin" % k)
        assert main(["--operation", "prove", "--witness-path", str(w), "--proof-path", str(dev)] + extra + common) == 0
        assert dev.read_bytes() == host.read_bytes()
        assert main(["--operation", "verify", "--proof-path", str(dev), "--parser", "host"] + common) == 0
        assert main(["--operation", "verify", "--proof-path", str(host)] + extra + common) == 0
    assert main(["--operation", "oneshot-zk", "--witness-path", str(w), "--parser", "device"] + common) == 0
    for ev in (["--evaluator", "gpu"], ["--evaluator", "gpu", "--compiler", "device"], ["--evaluator", "stream", "--max-chunk-ops", "256"],
               ["--evaluator", "stream", "--compact-wires", "--compiler", "device"], []):
        assert main(["--operation", "oneshot", "--witness-path", str(w), "--parser", "device"] + ev + common) == 0
    # a rejected proof stays rejected, and a statement that does not hold is reported
    bad = bytearray(host.read_bytes())
    bad[-1] ^= 1
    host.write_bytes(bytes(bad))
    assert main(["--operation", "verify", "--proof-path", str(host), "--parser", "device"] + common) == 1
    e.write_text("".join(str((9 >> i) & 1) for i in range(64)))
    for ev in ("gpu", "stream"):
        with pytest.raises(SystemExit):
            main(["--operation", "oneshot", "--evaluator", ev, "--witness-path", str(w), "--parser", "device"] + common)
