"""rv_ops_compact_wires (the host sweep; no GPU) against the rule as plain Python (tests/compact_ref.py), byte for byte; the proof of
the compacted list against the proof of the original through the CPU oracle; idempotence, in-place use and the error codes."""
import ctypes as C

import numpy as np
import pytest

import circuits
import compact_cases
import compact_ref
from reverie_amd.ops import OP_DTYPE

CORPUS = compact_cases.corpus()
ERRORS = compact_cases.error_cases()
INFO_FIELDS = ("z64_wires", "gf2_wires", "gf2_pinned", "gf2_zero_wire", "z64_zero_wire", "gf2_values", "z64_values")


@pytest.fixture(scope="module")
def L():
    import os

    from reverie_amd import _lib

    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__

        __graft_entry__.build()
    return _lib


def sweep(L, prog, wc, out=None):
    """-> (rc, out array, info dict) of one rv_ops_compact_wires call; out None: a fresh array filled with 0xA5 and 3 records longer than the list"""
    prog = np.ascontiguousarray(prog)
    if out is None:
        out = np.frombuffer(b"\xA5" * ((len(prog) + 3) * OP_DTYPE.itemsize), OP_DTYPE).copy()
    ci = L.CompactInfo()
    rc = L.lib().rv_ops_compact_wires(prog.ctypes.data_as(C.c_void_p), len(prog), int(wc[0]), int(wc[1]), out.ctypes.data_as(C.c_void_p), C.byref(ci))
    return rc, out, {k: int(getattr(ci, k)) for k in INFO_FIELDS}


@pytest.mark.parametrize("name,prog,wc", CORPUS, ids=[c[0] for c in CORPUS])
def test_sweep_equals_reference(L, name, prog, wc):
    rc_ref, want, counts, info = compact_ref.compact(prog, wc)
    assert rc_ref == 0
    before = prog.tobytes()
    rc, out, got = sweep(L, prog, wc)
    assert rc == 0
    assert prog.tobytes() == before
    assert out[:len(prog)].tobytes() == want.tobytes()
    assert out[len(prog):].tobytes() == b"\xA5" * (3 * OP_DTYPE.itemsize)  # (nothing behind the list is written)
    assert got == info and (got["z64_wires"], got["gf2_wires"]) == counts
    # the new list is a program under the new counts, and compacting it again changes nothing
    rc2, out2, got2 = sweep(L, want, counts)
    assert rc2 == 0 and out2[:len(prog)].tobytes() == want.tobytes()
    assert (got2["z64_wires"], got2["gf2_wires"]) == counts
    # in place
    buf = prog.copy()
    rc3, _, got3 = sweep(L, buf, wc, out=buf)
    assert rc3 == 0 and buf.tobytes() == want.tobytes() and got3 == info


def test_reference_figures():
    """the figures of the rule's description: the SSA layered circuit goes from 3 392 GF(2) wires to 298, a mixed program keeps its 64 pinned"""
    prog, _, wc, _ = circuits.layered_gf2(n_in=64, width=256, layers=12, fold_to=16)
    assert wc == (0, 3392)
    assert compact_ref.compact(prog, wc)[2] == (0, 298)
    prog, _, _, wc = circuits.random_mixed(np.random.default_rng(3))
    info = compact_ref.compact(prog, wc)[3]
    assert info["gf2_pinned"] == 64 and info["gf2_wires"] <= 90 and info["z64_wires"] <= 13


def test_python_front_end(L):
    import reverie_amd

    prog, _, wc, _ = circuits.layered_gf2(n_in=64, width=256, layers=12, fold_to=16)
    out, counts, info = reverie_amd.compact_wires(prog, wc)
    assert counts == (0, 298) and info["gf2_values"] == 3392 and out.dtype == OP_DTYPE
    assert out.tobytes() == compact_ref.compact(prog, wc)[1].tobytes()
    out2, counts2, _ = reverie_amd.compact_wires(prog.tolist())  # (op tuples; the counts from largest_wires)
    assert counts2 == counts and out2.tobytes() == out.tobytes()
    with pytest.raises(reverie_amd.ReverieError) as e:
        reverie_amd.compact_wires(prog, (0, 100))
    assert e.value.code == 3


def parity_programs():
    out = []
    for s in range(4):
        p, w, c = circuits.random_gf2(np.random.default_rng(40 + s), n_wires=8 + 9 * s)
        out.append((f"random_gf2_{s}", p, w, [], c))
    for s in range(3):
        p, w2, w64, c = circuits.random_mixed(np.random.default_rng(60 + s), n_gates=120)
        out.append((f"random_mixed_{s}", p, w2, w64, c))
    p, w, c, _ = circuits.layered_gf2(n_in=64, width=256, layers=12, fold_to=16)
    out.append(("layered_gf2_ssa", p, w, [], c))
    return out


PARITY = parity_programs()


@pytest.mark.parametrize("name,prog,w2,w64,wc", PARITY, ids=[c[0] for c in PARITY])
def test_oracle_proof_parity(L, oracle, rule_seeds, name, prog, w2, w64, wc):
    rc, out, info = sweep(L, prog, wc)
    assert rc == 0
    new, counts = out[:len(prog)].copy(), (info["z64_wires"], info["gf2_wires"])
    want = oracle.prove(prog, w2, w64, wc, rule_seeds)
    assert oracle.prove(new, w2, w64, counts, rule_seeds) == want
    assert oracle.verify(new, counts, want, strict=True)


@pytest.mark.parametrize("name,prog,wc,code", ERRORS, ids=[c[0] for c in ERRORS])
def test_errors(L, oracle, name, prog, wc, code):
    want = code if code is not None else compact_cases.oracle_code(oracle, prog, wc)
    assert want in (3, 5)
    assert compact_ref.compact(prog, wc)[0] == want
    rc, out, _ = sweep(L, prog, wc)
    assert rc == want
    assert out.tobytes() == b"\xA5" * len(out.tobytes())  # untouched
    buf = prog.copy()
    assert sweep(L, buf, wc, out=buf)[0] == want and buf.tobytes() == prog.tobytes()


def test_arguments(L):
    prog, wc = compact_cases.chain(10)
    two = np.concatenate([prog, prog])
    ci = L.CompactInfo()
    f = L.lib().rv_ops_compact_wires
    p = two.ctypes.data
    assert f(None, 3, 0, 1, C.c_void_p(p), C.byref(ci)) == 9
    assert f(C.c_void_p(p), 3, 0, 1, None, C.byref(ci)) == 9
    assert f(C.c_void_p(p), len(prog), wc[0], wc[1], C.c_void_p(p + OP_DTYPE.itemsize), C.byref(ci)) == 9  # a partial overlap
    assert f(C.c_void_p(p), len(prog), wc[0], wc[1], C.c_void_p(p + len(prog) * OP_DTYPE.itemsize), None) == 0  # (info is optional)
    assert two[len(prog):].tobytes() == compact_ref.compact(prog, wc)[1].tobytes()
    assert f(None, 0, 0, 0, None, C.byref(ci)) == 0 and ci.gf2_wires == 0
