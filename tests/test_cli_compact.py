"""`python -m reverie_amd --compact-wires`: prove / verify / oneshot-zk and the streamed oneshot on a Bristol circuit (SSA by nature).
The proof is the one made without the flag (the command line draws its seeds from the OS: the tests put fixed ones in their place)."""
import pytest

import bristol_gen
import compact_ref
from reverie_amd import bristol
from reverie_amd.__main__ import build_parser, load_program, main


def adder_files(tmp_path, a=0x0123456789ABCDEF, b=0xFEDCBA9876543210):
    p = tmp_path / "adder.txt"
    p.write_text(bristol_gen.adder64())
    w = tmp_path / "wit.txt"
    w.write_text(" ".join(str((a >> i) & 1) for i in range(64)) + "\n" + " ".join(str((b >> i) & 1) for i in range(64)))
    e = tmp_path / "exp.txt"
    e.write_text("".join(str((((a + b) & (2**64 - 1)) >> i) & 1) for i in range(64)))
    return p, w, e


def test_flag_and_bristol_front_end(tmp_path):
    assert build_parser().parse_args(["--operation", "prove", "--compact-wires"]).compact_wires
    assert not build_parser().parse_args(["--operation", "prove"]).compact_wires
    p, w, e = adder_files(tmp_path)
    with pytest.raises(SystemExit):  # (only the streamed oneshot keeps a wire store)
        main(["--operation", "oneshot", "--compact-wires", "--program-path", str(p), "--witness-path", str(w)])
    exp = [int(c) for c in e.read_text()]
    prog, info = bristol.parse(p.read_text(), expected_outputs=exp)
    small, sinfo = bristol.parse(p.read_text(), expected_outputs=exp, compact=True)
    rc, want, counts, cinfo = compact_ref.compact(prog, info["wire_counts"])
    assert rc == 0 and small.tobytes() == want.tobytes()
    assert sinfo["wire_counts"] == counts and sinfo["gf2_wires"] == counts[1] and sinfo["ssa_wire_counts"] == info["wire_counts"]
    assert sinfo["compact"] == cinfo and counts[1] < info["gf2_wires"]
    assert "compact" not in info and load_program(str(p), "auto", str(e))[1] == info["wire_counts"]  # (the default is the parser's numbering)


@pytest.mark.gpu
def test_cli_compact_roundtrip(tmp_path, capsys, monkeypatch, rule_seeds):
    from reverie_amd.proof import Proof

    p, w, e = adder_files(tmp_path)
    plain_new = Proof.new
    monkeypatch.setattr(Proof, "new", staticmethod(lambda circuit, wit_gf2, wit_z64, *a, **k: plain_new(circuit, wit_gf2, wit_z64, *a, **{**k, "seeds": rule_seeds})))
    common = ["--program-path", str(p), "--expected-outputs-path", str(e)]
    ssa, small = tmp_path / "proof_ssa.bin", tmp_path / "proof_compact.bin"
    assert main(["--operation", "prove", "--witness-path", str(w), "--proof-path", str(ssa)] + common) == 0
    assert "compact-wires" not in capsys.readouterr().err
    assert main(["--operation", "prove", "--witness-path", str(w), "--proof-path", str(small), "--compact-wires"] + common) == 0
    prog, wc = load_program(str(p), "auto", str(e))
    counts = compact_ref.compact(prog, wc)[2]
    assert "compact-wires: wire counts (z64, gf2) %s -> %s" % (wc, counts) in capsys.readouterr().err
    assert small.read_bytes() == ssa.read_bytes()
    for proof in (ssa, small):
        assert main(["--operation", "verify", "--proof-path", str(proof), "--compact-wires"] + common) == 0
        assert main(["--operation", "verify", "--proof-path", str(proof)] + common) == 0
    assert main(["--operation", "oneshot-zk", "--witness-path", str(w), "--compact-wires"] + common) == 0
    assert main(["--operation", "oneshot", "--evaluator", "stream", "--witness-path", str(w), "--compact-wires", "--max-chunk-ops", "256"] + common) == 0
    raw = tmp_path / "adder.rvops"
    raw.write_bytes(prog.tobytes())
    assert main(["--operation", "oneshot", "--evaluator", "stream", "--witness-path", str(w), "--compact-wires", "--program-path", str(raw)]) == 0
    # a rejected proof stays rejected
    bad = bytearray(ssa.read_bytes())
    bad[-1] ^= 1
    small.write_bytes(bytes(bad))
    assert main(["--operation", "verify", "--proof-path", str(small), "--compact-wires"] + common) == 1
    # a statement that does not hold is reported by the streamed evaluation of the compacted list too
    e.write_text("".join(str((9 >> i) & 1) for i in range(64)))
    with pytest.raises(SystemExit):
        main(["--operation", "oneshot", "--evaluator", "stream", "--witness-path", str(w), "--compact-wires"] + common)
