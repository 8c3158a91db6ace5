"""rv_verify_device / rv_verify_sections_device (reverie_amd.DeviceProof): Proof::verify on proof bytes that lie in GPU memory.

The contract: the answer -- a bool or an error code -- is rv_verify_ex's on a host copy of the same bytes, for every byte string;
a well-framed proof whose records pass check_records is verified where it lies (rv_hook_verify_device_paths counts the calls
that did, and the calls that fell back to the host verifier; rv_hook_verify_proof_bytes, the host verifier's upload counter,
must not move on the device path).

Golden circuits (zero-length vectors, vectors that end at every byte alignment, both domains), the altered-length catalogues of
tests/verify_length_cases.py against the oracle's answers (computed once per process, shared with test_gpu_verify_lengths.py),
the 4.8 MB proof of split_circuit() -- the size at which the host form changes its schedule --, flipped bytes, truncations,
wrong counts and the argument errors."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import proof_mutate
import verify_length_cases as cases
from conftest import GOLDEN, golden_ops
from reverie_amd.ops import OP_DTYPE, program
from test_gpu_verify_lengths import ENV, MALFORMED, MODES, Report, case, fused_eligible, got, rv, set_env  # noqa: F401 (case, rv: fixtures)
from test_verify_device_host import PRE, expected_table, sections_of, with_counts

pytestmark = pytest.mark.gpu

META = json.load(open(os.path.join(GOLDEN, "proofs.json")))
GOLDEN_NAMES = ("empty", "adder64", "gf2_mix", "z64_mix", "sizehint_mixed")
E_ARG = ("err", 9)


def upload(data: bytes):
    """the bytes in a fresh GPU tensor (torch's allocations start on 512-byte boundaries)"""
    import torch

    t = torch.frombuffer(bytearray(data), dtype=torch.uint8).cuda()
    assert t.data_ptr() % 16 == 0
    return t


def counters():
    """(device-path calls, fallback calls, proof bytes the host verifier uploaded)"""
    from reverie_amd import _lib

    out = (C.c_uint64 * 2)()
    assert _lib.lib().rv_hook_verify_device_paths(out) == 0
    return int(out[0]), int(out[1]), int(_lib.lib().rv_hook_verify_proof_bytes())


def device_answer(rv, circuit, dp, strict, path):
    """got(dp.verify), with the call's way asserted: path "device" (the upload counter still), "fallback" or "refused" (neither)"""
    d0, f0, b0 = counters()
    have = got(dp.verify, circuit, strict=strict)
    d1, f1, b1 = counters()
    assert (d1 - d0, f1 - f0) == {"device": (1, 0), "fallback": (0, 1), "refused": (0, 0)}[path], (path, have)
    if path != "fallback":
        assert b1 == b0, "a proof verified in device memory was uploaded"
    return have


def golden(name):
    m = META[name]
    ops = golden_ops(m)
    prog = program(ops) if ops else np.zeros(0, OP_DTYPE)
    proof = open(os.path.join(GOLDEN, f"proof_{name}.bin"), "rb").read()
    return prog, m["wit_gf2"], [int(x) for x in m["wit_z64"]], tuple(m["wire_counts"]), proof


@pytest.mark.parametrize("name", GOLDEN_NAMES)
def test_golden_proofs(rv, rule_seeds, name):
    prog, w2, w64, wc, proof = golden(name)
    c = rv.Circuit(prog, wc)
    try:
        dp = rv.DeviceProof(upload(proof))
        for strict in (True, False):
            assert device_answer(rv, c, dp, strict, "device") is True
        assert dp.comm == proof[:32] and bytes(dp.to_proof()) == proof
        # the sections rv_prove_device leaves, for the same seeds: the same proof, verified without being framed
        ds = rv.DeviceProof.new(c, w2, w64, seeds=rule_seeds)
        sec, lens = sections_of(proof)
        assert ds.lens == lens and ds.comm == proof[:32] and bytes(ds.tensor[:sum(lens)].cpu().numpy().tobytes()) == sec
        for strict in (True, False):
            assert device_answer(rv, c, ds, strict, "device") is True
        assert bytes(ds.to_proof()) == proof
        assert rv.DeviceProof.new(c, w2, w64).verify(c)  # (seeds from the OS)
    finally:
        c.close()


# ---- the altered-length catalogues: the oracle's answer, and the device path for everything the oracle does not call malformed
@pytest.mark.parametrize("name", cases.NAMES)
def test_altered_lengths(rv, case, monkeypatch, name):
    rep = Report(f"{name} rv_verify_device")
    if name == "Z":
        assert fused_eligible(rv, case["prog"], case["wc"], monkeypatch)
    proofs = [rv.DeviceProof(upload(data)) for _, data in case["entries"]]
    good = rv.DeviceProof(upload(case["good"]))
    n_device = 0
    for env in ENV[name]:
        set_env(monkeypatch, env)
        for strict, _ in MODES:
            assert device_answer(rv, case["circuit"], good, strict, "device") is True
        for (label, _), dp, want in zip(case["entries"], proofs, case["answers"]):
            for strict, k in MODES:
                path = "fallback" if want[k] == MALFORMED else "device"
                n_device += path == "device"
                rep.check(label, f"strict={strict} {env}", device_answer(rv, case["circuit"], dp, strict, path), want[k])
    assert n_device >= 20 * len(MODES) * len(ENV[name])
    rep.done()


@pytest.mark.parametrize("name", ("MIX", "Z"))
def test_altered_lengths_sections(rv, case, name):
    """the sections form on the catalogue's thin axis: the same records without comm and counts (entries with bytes behind the
    proof have no sections form)"""
    rep = Report(f"{name} rv_verify_sections_device")
    for i in case["thin"]:
        (label, data), want = case["entries"][i], case["answers"][i]
        if label.startswith("trailing"):
            continue
        sec, lens = sections_of(data)
        dp = rv.DeviceProof(sections=upload(sec), lens=lens, comm=data[:32])
        for strict, k in MODES:
            path = "fallback" if want[k] == MALFORMED else "device"
            rep.check(label, f"strict={strict}", device_answer(rv, case["circuit"], dp, strict, path), want[k])
    rep.done()


# ---- a proof above 4 MB
_split = {}
SPLIT_PARTS = [(d, v, g) for d in proof_mutate.DOMAINS for v in proof_mutate.VECTORS for g in proof_mutate.GROUPS]
SPLIT_PARTS += [("same", None, g) for g in proof_mutate.GROUPS]


@pytest.mark.parametrize("dom,vec,group", SPLIT_PARTS)
def test_large_proof(rv, oracle, rule_seeds, monkeypatch, dom, vec, group):
    """split_circuit(): 4.8 MB of online records, above the size from which the host form copies the proof on its second stream
    and splits the fused Z64 verifier's quad groups.  The good proof and the THIN_TARGETS catalogue, one domain, vector and
    group per case (and the same-length changes of a group in a case of their own)."""
    if not _split:
        prog, w64, wc = cases.split_circuit()
        good = oracle.prove(prog, [], w64, wc, rule_seeds)
        assert len(good) > 4 << 20
        _split.update(prog=prog, wc=wc, good=good, circuit=rv.Circuit(prog, wc))
    prog, wc, good, c = (_split[k] for k in ("prog", "wc", "good", "circuit"))
    dg = rv.DeviceProof(upload(good))
    for strict, _ in MODES:
        assert device_answer(rv, c, dg, strict, "device") is True
    targets = tuple(t for t in proof_mutate.THIN_TARGETS if t[1] == group)
    if dom == "same":
        entries = list(proof_mutate.catalogue(good, targets=targets, domains=(), gf2_items=cases.gf2_items(prog)))
    else:
        entries = list(proof_mutate.catalogue(good, targets=targets, domains=(dom,), vectors=(vec,), same_length=False))
    assert len(entries) >= 20
    answers = cases.answers(oracle, prog, wc, entries)
    rep = Report(f"SPLIT rv_verify_device {dom} {vec} g{group}")
    for (label, data), want in zip(entries, answers):
        dp = rv.DeviceProof(upload(data))
        for strict, k in MODES:
            path = "fallback" if want[k] == MALFORMED else "device"
            rep.check(label, f"strict={strict}", device_answer(rv, c, dp, strict, path), want[k])
    rep.done()


# ---- single bytes, truncations, counts, arguments
def test_flipped_bytes_truncations_counts(rv):
    prog, w2, w64, wc, proof = golden("gf2_mix")
    c = rv.Circuit(prog, wc)
    t = expected_table(proof)
    assert t[2] > 0  # (record 0 has a rec vector)
    player = (t[7] + 1) % 8  # a player record 0 opens
    flips = {"comm": 0, "key": t[0] + 16 * player, "rec": t[1], "seed": t[PRE] + 5 * 48}
    try:
        for what, at in flips.items():
            data = bytearray(proof)
            data[at] ^= 0xFF
            data = bytes(data)
            for strict in (True, False):
                assert rv.Proof(data).verify(c, strict=strict) is False, what
                assert device_answer(rv, c, rv.DeviceProof(upload(data)), strict, "device") is False, what
        # truncated: rv_verify_ex's code, through the fallback
        for n in (31, 32, 40, 40 + 129 + 8 + 3, len(proof) - 1):
            for strict in (True, False):
                want = got(rv.Proof(proof[:n]).verify, c, strict=strict)
                assert want == MALFORMED
                assert device_answer(rv, c, rv.DeviceProof(upload(proof[:n])), strict, "fallback") == want, n
        # wrong repetition counts (39 and 41 records, framed as such): `false`, not an error
        comm, good = proof_mutate.parse(proof)
        for n in (39, 41):
            for which in ((0,), (1,), (0, 1)):
                doms = proof_mutate._copy(good)
                for d in which:
                    doms[d] = ((doms[d][0] + doms[d][0][-1:])[:n], doms[d][1])
                data = proof_mutate.serialise(comm, doms)
                for strict in (True, False):
                    assert rv.Proof(data).verify(c, strict=strict) is False
                    assert device_answer(rv, c, rv.DeviceProof(upload(data)), strict, "fallback") is False, (n, which)
        # ... and counts that lie about what follows them: whatever rv_verify_ex makes of the bytes
        for value in (39, 41):
            for which in range(4):
                data = with_counts(proof, [which], value)
                for strict in (True, False):
                    want = got(rv.Proof(data).verify, c, strict=strict)
                    assert device_answer(rv, c, rv.DeviceProof(upload(data)), strict, "fallback") == want, (value, which)
    finally:
        c.close()


def test_argument_errors(rv):
    import torch

    from reverie_amd import _lib

    prog, w2, w64, wc, proof = golden("adder64")
    c = rv.Circuit(prog, wc)
    L = _lib.lib()
    try:
        one_off = upload(b"\0" + proof)[1:]  # the proof's bytes, one byte off the allocation's boundary
        assert device_answer(rv, c, rv.DeviceProof(one_off), True, "refused") == E_ARG
        sec, lens = sections_of(proof)
        assert device_answer(rv, c, rv.DeviceProof(sections=upload(b"\0" + sec)[1:], lens=lens, comm=proof[:32]), True, "refused") == E_ARG
        # host memory
        ok = C.c_int(7)
        host = np.frombuffer(proof, np.uint8).copy()
        before = counters()
        assert L.rv_verify_device(c.ctx.handle, c.handle, host.ctypes.data_as(C.c_void_p), len(proof), 0, C.byref(ok)) == 9
        assert L.rv_verify_sections_device(c.ctx.handle, c.handle, host.ctypes.data_as(C.c_void_p), host.ctypes.data_as(C.c_void_p),
                                           (C.c_size_t * 4)(*lens), 0, C.byref(ok)) == 9
        t = upload(proof)
        assert L.rv_verify_device(c.ctx.handle, c.handle, None, len(proof), 0, C.byref(ok)) == 9
        assert L.rv_verify_device(c.ctx.handle, c.handle, C.c_void_p(t.data_ptr()), len(proof), 3, C.byref(ok)) == 9  # both flag bits
        assert L.rv_verify_device(c.ctx.handle, c.handle, C.c_void_p(t.data_ptr()), len(proof), 0, None) == 9
        assert counters() == before
        # Python: a round trip, and what is refused before any library call
        dp = rv.DeviceProof(t)
        assert dp.verify(c) and dp.verify(c, strict=False) and bytes(dp.to_proof()) == proof and dp.to_proof().verify(c)
        with pytest.raises(TypeError):
            rv.DeviceProof(torch.frombuffer(bytearray(proof), dtype=torch.uint8))
        with pytest.raises(ValueError):
            rv.DeviceProof(t.view(2, -1))
        with pytest.raises(TypeError):
            dp.verify(prog)
        assert counters()[:2] == (before[0] + 2, before[1])
    finally:
        c.close()
