"""rv_link, the host definition of the linker (no GPU): its bytes and info against the numpy model of tests/link_ref.py (which
shares no code with it) on every case of tests/link_cases.py, the error rule case by case, a chain of adders evaluated in the clear,
and the kernels' order of work -- reverie_amd/csrc/link.h run as plain CPU loops -- in a stand-alone program built with
-fsanitize=address,undefined (tests/link_model.cpp)."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import bristol_gen
import link_cases as lc
import link_ref
from conftest import ROOT


@pytest.fixture(scope="module")
def L():
    from reverie_amd import _lib

    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__

        __graft_entry__.build()
    return _lib.lib()


@pytest.fixture(scope="module")
def T(L):
    out = (C.c_uint32 * 2)()
    assert L.rv_hook_link_tiles(out) == 0
    return int(out[0])


def host_link(spec):
    """-> (code, ops, info) through reverie_amd.link"""
    from reverie_amd import ReverieError

    try:
        ops, info = lc.to_netlist(spec).link_host()
    except ReverieError as e:
        return e.code, None, None
    return 0, ops, info


def test_symbols_exported_and_bound(L):
    import reverie_amd
    from reverie_amd import _lib, link

    hdr = open(os.path.join(ROOT, "include", "reverie_amd.h")).read()
    for name in ("rv_link", "rv_link_plan_create", "rv_link_plan_info", "rv_link_plan_emit", "rv_link_plan_destroy", "rv_hook_link_tiles"):
        assert name in _lib.SYMBOLS and name in _lib.ARGTYPES
        assert getattr(L, name).argtypes is not None
        assert re.search(r"\b" + name + r"\s*\(", hdr), name
    assert C.sizeof(_lib.LinkInfo) == 48 and C.sizeof(_lib.LinkPiece) == 32 and C.sizeof(_lib.LinkBlock) == 32 and C.sizeof(_lib.LinkDesc) == 96
    assert L.rv_abi_version() == 8  # (calls were added, nothing changed)
    out = (C.c_uint32 * 2)()
    assert L.rv_hook_link_tiles(out) == 0 and L.rv_hook_link_tiles(None) == link_ref.ARG
    assert out[0] == 256 and out[1] >= out[0]
    assert reverie_amd.Netlist is link.Netlist and reverie_amd.Block is link.Block and reverie_amd.LinkPlan is link.LinkPlan
    assert link.WITNESS == link_ref.WITNESS == 0xFFFFFFFF


def test_cases_are_the_issue_s(T):
    """the case list covers what it says: the totals around the tile, many and empty instances, every opcode"""
    cases = dict(lc.ok_cases(T))
    totals = {link_ref.check(s)[1]["n_ops"] for s in cases.values()}
    assert {T - 1, T, T + 1, 2 * T - 1, 2 * T, 2 * T + 1} <= totals and 0 in totals
    assert len(cases["600-instances-of-0-1-3"].block_of) == 600
    every = cases["every-opcode"].blocks[0][0]
    assert {(d, o) for d in (0, 1) for o in range(10)} <= set(zip(every["domain"].tolist(), every["opcode"].tolist())) and (every["domain"] == 2).any()
    assert 36 <= link_ref.check(cases["forty"])[1]["n_ops"] <= 48


def test_bytes_and_info_are_the_model_s(L, T):
    for name, spec in lc.ok_cases(T):
        code, want, winfo = link_ref.link(spec)
        assert code == 0, name
        rc, ops, info = host_link(spec)
        assert rc == 0, (name, rc)
        assert ops.tobytes() == want.tobytes(), name
        assert info == winfo, (name, info, winfo)
        _, only = lc.to_netlist(spec).link_host(info_only=True)
        assert only == winfo, name


@pytest.mark.parametrize("name,spec,code", lc.bad_cases(), ids=[c[0] for c in lc.bad_cases()])
def test_codes(L, name, spec, code):
    rc, ops, info = host_link(spec)
    assert rc == code and ops is None and info is None


def test_argument_errors(L):
    from reverie_amd import _lib

    info, ops = _lib.LinkInfo(), C.c_void_p()
    d = _lib.LinkDesc()
    assert L.rv_link(None, C.byref(ops), C.byref(info)) == link_ref.ARG
    assert L.rv_link(C.byref(d), C.byref(ops), None) == link_ref.ARG
    assert L.rv_link(C.byref(d), C.byref(ops), C.byref(info)) == 0 and info.n_ops == 0  # (the empty netlist)
    L.rv_free(ops)
    for field in ("n_blocks", "n_instances", "n_bindings", "n_head", "n_tail"):
        d = _lib.LinkDesc()
        setattr(d, field, 1)
        assert L.rv_link(C.byref(d), C.byref(ops), C.byref(info)) == link_ref.ARG and not ops
    blk = (_lib.LinkBlock * 1)(_lib.LinkBlock(None, 1, 0, 0))
    d = _lib.LinkDesc(blk, 1)
    assert L.rv_link(C.byref(d), C.byref(ops), C.byref(info)) == link_ref.ARG
    d = _lib.LinkDesc(None, 0, None, 1 << 31)  # decided before the arrays are looked at
    assert L.rv_link(C.byref(d), C.byref(ops), C.byref(info)) == link_ref.ARG
    one = np.zeros(1, np.uint32)
    d = _lib.LinkDesc(None, 0, one.ctypes.data, 1 << 31)
    assert L.rv_link(C.byref(d), C.byref(ops), C.byref(info)) == link_ref.UNSUPPORTED


def test_adder_chain_adds(L):
    nl, outputs, tail, bits, total = lc.adder_chain()
    assert total == sum(int("".join(map(str, bits[64 * k:64 * k + 64][::-1])), 2) for k in range(9)) % (1 << 64)
    nl.set_tail(tail(total))
    ops, info = nl.link_host()
    assert info["n_instances"] == 8 and info["n_input_gf2"] == len(bits) == 64 * 9 and info["n_input_z64"] == 0
    assert info["n_ops"] == len(ops) == 8 * len(nl.blocks[0].ops) + 128
    values = bristol_gen.evaluate(ops, bits)
    assert sum(values[o] << k for k, o in enumerate(outputs)) == total
    nl2, _, tail2, bits2, total2 = lc.adder_chain()
    nl2.set_tail(tail2(total2 ^ 4))
    with pytest.raises(ValueError, match="AssertZero"):
        bristol_gen.evaluate(nl2.link_host()[0], bits2)


def test_model_under_sanitizers(L, T, tmp_path):
    """the stand-alone program: clean under AddressSanitizer and UBSan; for every case the kernels' order of work gives rv_link's
    code, info and bytes (the program compares) and those are the numpy model's (compared here, by digest); every range of the small
    cases gives rv_link's bytes and Input counts"""
    exe = str(tmp_path / "link_model")
    csrc = os.path.join(ROOT, "reverie_amd", "csrc")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", csrc,
                           os.path.join(ROOT, "tests", "link_model.cpp"), os.path.join(csrc, "link.cpp"), "-o", exe])
    whole = [(n, s, 0) for n, s in lc.ok_cases(T)] + lc.bad_cases()
    paths, small = [], []
    for k, (name, spec, code) in enumerate(whole):
        path = str(tmp_path / f"{k:03d}-{name}.net")
        with open(path, "wb") as f:
            f.write(lc.to_file(spec))
        n_ops = link_ref.check(spec)[1]["n_ops"] if code == 0 else 0
        (small if code == 0 and n_ops < 64 else paths).append(path)
    run = subprocess.run([exe] + paths + ["--ranges"] + small, capture_output=True, text=True)
    assert run.returncode == 0 and "Sanitizer" not in run.stderr and "runtime error" not in run.stderr, (run.stdout[-2000:], run.stderr[-2000:])
    lines = run.stdout.split("\n")
    assert lines[-2] == "bad 0"
    answers = {ln.split()[0]: ln.split()[1:] for ln in lines if re.match(r"\d\d\d-", ln)}
    assert len(answers) == len(whole)
    for k, (name, spec, code) in enumerate(whole):
        rc, n_ops, digest = answers[f"{k:03d}-{name}.net"]
        assert int(rc) == code, name
        if code == 0:
            want = link_ref.link(spec)[1]
            assert int(n_ops) == len(want) and int(digest, 16) == lc.fnv(want.tobytes()), name
    counts = {ln.split()[1]: int(ln.split()[2]) for ln in lines if ln.startswith("ranges ")}
    sizes = {os.path.basename(p): link_ref.check(whole[int(os.path.basename(p)[:3])][1])[1]["n_ops"] for p in small}
    assert counts == {p: (n + 1) * (n + 2) // 2 for p, n in sizes.items()} and max(sizes.values()) >= 36
