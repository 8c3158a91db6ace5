"""rv_bristol_header and bristol.dumps (host only, no GPU): the header code the host parser and the device parser share, and the
writer the parser benchmark and the device parser's tests use."""
import numpy as np
import pytest

import bristol_cases as bc
import bristol_gen
from reverie_amd import _lib, bristol
from reverie_amd.ops import GF2, OP_DTYPE, Z64, program

HEADER_KEYS = ("n_gates", "n_wires", "n_inputs", "n_outputs")
TEXTS = [(n, t, None, f) for n, t, f in bc.well_formed() + bc.boundary_texts()] + [c[:4] for c in bc.error_texts()]


def test_abi_version_stays_8():
    assert _lib.lib().rv_abi_version() == 8


@pytest.mark.parametrize("name,text,expected,fmt,code", bc.error_texts(), ids=[c[0] for c in bc.error_texts()])
def test_error_corpus_has_the_stated_codes(name, text, expected, fmt, code):
    """the corpus' codes are the host parser's (what the device parser is compared with)"""
    assert bc.host_parse(text, expected, fmt)[0] == code


@pytest.mark.parametrize("name,text,expected,fmt", TEXTS, ids=[c[0] for c in TEXTS])
def test_header_agrees_with_the_parser(name, text, expected, fmt):
    rc, n_ops, _, info = bc.host_parse(text, None, fmt)
    hrc, hinfo, off = bc.host_header(text, fmt)
    if rc == 0:
        assert hrc == 0
        assert {k: hinfo[k] for k in HEADER_KEYS} == {k: info[k] for k in HEADER_KEYS}
        assert all(v == 0 for k, v in hinfo.items() if k not in HEADER_KEYS)
        # the gate lines begin at the offset: the text's gates alone, behind a header of the same counts, parse to the same records
        gates = text[off:]
        again = b"%d %d\n1 %d\n1 %d\n" % (info["n_gates"], info["n_wires"], info["n_inputs"], info["n_outputs"]) + gates
        assert bc.host_parse(again, None, 1)[2] == bc.host_parse(text, None, fmt)[2]
        assert off == len(text) or text[off - 1:off] == b"\n"
    elif hrc != 0:
        assert hrc == rc  # a header defect: the parser's code
    else:
        # the header is sound, so the defect is a gate line's: the same text with no gate line claimed parses
        assert hinfo["n_gates"] > 0


def test_header_defects_carry_the_parsers_code():
    for text, fmt in ((b"", 0), (b"3\n", 0), (b"1 4\n", 0), (b"1 4\nx 4\n", 0), (b"1 4\n1 5\n1 1\n2 1 0 1 2 XOR\n", 0),
                      (b"1 4\n1 2\n1 5\n2 1 0 1 2 XOR\n", 0), (b"1 4294967296\n1 4\n1 1\n", 0), (b"99 16\n1 4\n1 2\n2 1 0 1 4 XOR\n", 0),
                      (b"1 4\n2 1 1 1\n1 1\n2 1 0 1 2 XOR\n", 2), (b"1 4\n2 1 1\n2 1 0 1 2 XOR\n", 1)):
        rc = bc.host_parse(text, None, fmt)[0]
        assert rc != 0
        assert bc.host_header(text, fmt)[0] == rc, text


def test_header_null_arguments():
    import ctypes as C

    L = _lib.lib()
    bi, off = _lib.BristolInfo(), C.c_size_t()
    t = np.frombuffer(b"0 4\n1 4\n1 2\n", np.uint8)
    assert L.rv_bristol_header(None, 0, 0, C.byref(bi), C.byref(off)) == bc.ARG
    assert L.rv_bristol_header(C.c_void_p(t.ctypes.data), t.size, 0, None, C.byref(off)) == bc.ARG
    assert L.rv_bristol_header(C.c_void_p(t.ctypes.data), t.size, 0, C.byref(bi), None) == bc.ARG


def test_header_needs_no_more_than_the_first_gate_line():
    text = bc.well_formed()[4][1]  # the ambiguous second line, read as Fashion
    assert bc.well_formed()[4][0] == "ambiguous-fashion"
    rc, info, off = bc.host_header(text)
    first_gate_end = text.index(b"\n", off) + 1
    import ctypes as C

    bi, o2 = _lib.BristolInfo(), C.c_size_t()
    buf = np.frombuffer(text, np.uint8)
    assert _lib.lib().rv_bristol_header(C.c_void_p(buf.ctypes.data), first_gate_end, 0, C.byref(bi), C.byref(o2)) == 0
    assert (int(bi.n_inputs), int(bi.n_outputs), int(o2.value)) == (info["n_inputs"], info["n_outputs"], off)


def _random_bristol_program(n_gates, seed, n_in=6):
    rng = np.random.default_rng(seed)
    ops = [GF2.Input(i) for i in range(n_in)]
    w = n_in
    for _ in range(n_gates):
        a, b = (int(x) for x in rng.integers(0, w, 2))
        k = int(rng.integers(0, 5))
        ops.append((GF2.Add(w, a, b), GF2.Mul(w, a, b), GF2.AddConst(w, a, 1), GF2.AddConst(w, a, 0), GF2.Const(w, int(rng.integers(0, 2))))[k])
        w += 1
    return program(ops)


def test_dumps_round_trip_adder64():
    prog, info = bristol.parse(bristol_gen.adder64())
    text = bristol.dumps(prog, info["n_outputs"])
    again, info2 = bristol.parse(text)
    assert again.tobytes() == prog.tobytes()
    assert info2 == info


@pytest.mark.parametrize("n_gates,seed", [(0, 1), (1, 2), (97, 3), (1000, 4)])
def test_dumps_round_trip_random(n_gates, seed):
    prog = _random_bristol_program(n_gates, seed)
    again, info = bristol.parse(bristol.dumps(prog, 1))
    assert again.tobytes() == prog.tobytes()
    assert (info["n_inputs"], info["n_outputs"], info["n_gates"]) == (6, 1, n_gates)


@pytest.mark.parametrize("op", [Z64.Add(2, 0, 1), GF2.AssertZero(0), GF2.Sub(2, 0, 1), GF2.Random(2), GF2.AddConst(2, 0, 2)],
                         ids=["z64", "assert-zero", "sub", "random", "addconst-2"])
def test_dumps_refuses_what_bristol_cannot_say(op):
    with pytest.raises(ValueError):
        bristol.dumps(program([GF2.Input(0), GF2.Input(1), op]))


def test_dumps_refuses_b2a_and_misplaced_inputs():
    from reverie_amd.ops import B2A

    with pytest.raises(ValueError):
        bristol.dumps(program([GF2.Input(i) for i in range(64)] + [B2A(0, 0)]))
    with pytest.raises(ValueError):
        bristol.dumps(program([GF2.Input(0), GF2.Add(1, 0, 0), GF2.Input(2)]))
    with pytest.raises(ValueError):
        bristol.dumps(program([GF2.Input(1), GF2.Input(0)]))


def test_parse_device_and_dumps_are_exported():
    assert callable(bristol.parse_device) and callable(bristol.dumps) and callable(bristol.header)
    assert OP_DTYPE.itemsize == 24
