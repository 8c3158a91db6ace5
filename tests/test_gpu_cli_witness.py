"""`python -m reverie_amd --witness-parser device` on the GPU: the witness file parsed there (rv_witness_parse_device) and, with
--witness-window-mb under --stream, read in windows as the pieces ask for bits; the proofs verify, the oracle accepts them, and
oneshot prints what it prints with the host parser."""
import numpy as np
import pytest

import bristol_gen
from reverie_amd.__main__ import load_program, main

pytestmark = pytest.mark.gpu


@pytest.fixture()
def adder(tmp_path):
    """the 64-bit adder, a witness file with blanks, CR LF and a comment in it, the expected outputs, and a wrong witness"""
    p = tmp_path / "adder.txt"
    p.write_text(bristol_gen.adder64())
    a, b = 0x0123456789ABCDEF, 0xFEDCBA9876543210
    w = tmp_path / "wit.txt"
    w.write_bytes(b"a:\r\n" + " ".join(str((a >> i) & 1) for i in range(64)).encode() + b"\r\nb:\r\n" + " ".join(str((b >> i) & 1) for i in range(64)).encode())
    bad = tmp_path / "bad.txt"
    bad.write_text("".join(str((a >> i) & 1) for i in range(64)) + "\n" + "".join(str(((b + 1) >> i) & 1) for i in range(64)))
    e = tmp_path / "exp.txt"
    e.write_text("".join(str((((a + b) & (2**64 - 1)) >> i) & 1) for i in range(64)))
    return {"common": ["--program-path", str(p), "--expected-outputs-path", str(e)], "program": str(p), "expected": str(e), "witness": str(w),
            "bad": str(bad), "dir": tmp_path}


def test_prove_with_the_device_parser_then_verify(adder, capsys, oracle):
    out = adder["dir"] / "proof.bin"
    common = adder["common"]
    assert main(["--operation", "prove", "--witness-path", adder["witness"], "--proof-path", str(out), "--witness-parser", "device"] + common) == 0
    assert main(["--operation", "verify", "--proof-path", str(out)] + common) == 0
    assert main(["--operation", "oneshot-zk", "--witness-path", adder["witness"], "--witness-parser", "device"] + common) == 0
    txt = capsys.readouterr().out
    assert txt.count("Ok(())") == 3 and "Verifying Proof" in txt
    prog, wc = load_program(adder["program"], "auto", adder["expected"])
    assert oracle.verify(prog, wc, out.read_bytes())


def test_prove_with_program_and_witness_parsed_on_the_gpu(adder, capsys, oracle):
    """the program parsed and compiled on the GPU too: nothing of the statement passes through host arrays"""
    out = adder["dir"] / "proof.bin"
    common = adder["common"]
    prog, wc = load_program(adder["program"], "auto", adder["expected"])
    assert main(["--operation", "prove", "--witness-path", adder["witness"], "--proof-path", str(out), "--witness-parser", "device", "--parser", "device",
                 "--compiler", "device"] + common) == 0
    assert oracle.verify(prog, wc, out.read_bytes())


def test_oneshot_prints_the_same_with_both_parsers(adder, capsys):
    outs = []
    for parser in ("host", "device"):
        assert main(["--operation", "oneshot", "--evaluator", "gpu", "--witness-path", adder["witness"], "--witness-parser", parser] + adder["common"]) == 0
        outs.append(capsys.readouterr().out)
    assert outs[0] == outs[1] and "Evaluating program in cleartext" in outs[0] and outs[0].rstrip().endswith("()")
    msgs = []
    for parser in ("host", "device"):
        with pytest.raises(SystemExit) as e:
            main(["--operation", "oneshot", "--evaluator", "gpu", "--witness-path", adder["bad"], "--witness-parser", parser] + adder["common"])
        msgs.append(str(e.value.code))
        capsys.readouterr()
    assert msgs[0] == msgs[1] and "assertion failed: AssertZero at op" in msgs[0]
    # --evaluator auto with the device parser evaluates on the GPU; --evaluator stream reads the tensor piece by piece
    for extra in ([], ["--evaluator", "stream"], ["--evaluator", "stream", "--witness-window-mb", "1"]):
        assert main(["--operation", "oneshot", "--witness-path", adder["witness"], "--witness-parser", "device"] + extra + adder["common"]) == 0
        assert capsys.readouterr().out == outs[0]


def test_stream_with_witness_windows(adder, capsys, oracle):
    out = adder["dir"] / "streamed.bin"
    common = adder["common"]
    assert main(["--operation", "prove", "--stream", "--witness-path", adder["witness"], "--proof-path", str(out), "--witness-parser", "device",
                 "--witness-window-mb", "1"] + common) == 0
    assert main(["--operation", "verify", "--stream", "--proof-path", str(out)] + common) == 0
    assert main(["--operation", "verify", "--proof-path", str(out)] + common) == 0  # (a streamed proof verifies without --stream alike)
    assert capsys.readouterr().out.count("Ok(())") == 3
    prog, wc = load_program(adder["program"], "auto", adder["expected"])
    assert oracle.verify(prog, wc, out.read_bytes())
    # without the windows: the whole tensor, sliced by the pieces
    assert main(["--operation", "oneshot-zk", "--stream", "--witness-path", adder["witness"], "--witness-parser", "device"] + common) == 0
    assert capsys.readouterr().out.count("Ok(())") == 1
    # a witness file that ends one bit early
    short = adder["dir"] / "short.txt"
    short.write_bytes(np.frombuffer(b"01" * 63 + b"0\n", np.uint8).tobytes())
    from reverie_amd import ReverieError

    with pytest.raises(ReverieError) as e:
        main(["--operation", "prove", "--stream", "--witness-path", str(short), "--proof-path", str(out), "--witness-parser", "device",
              "--witness-window-mb", "1"] + common)
    assert e.value.code == 2
