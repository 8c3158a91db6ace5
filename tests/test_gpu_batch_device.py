"""rv_prove_batch_device / rv_verify_batch_device (reverie_amd.prove_batch_device, verify_batch_device): the batch entry points
for proofs that stay in GPU memory.

The prover's contract: bytes [b * stride, b * stride + proof_len) of the caller's buffer are rv_prove_batch's proof b for the same
witnesses and seeds, on every path (one pass, chunks, proof after proof).  The verifier's: the return code and every ok[b] are
rv_verify_batch's on host copies of the same bytes, for every byte string; rv_hook_verify_batch_device_paths tells which way each
proof went (one pass on the device, the single-proof device verifier, a host copy).

Golden circuits only (tens of gates, both domains, B2A, zero-length vectors), plus the altered-length catalogues of
tests/verify_length_cases.py that test_gpu_verify_lengths.py shares."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import proof_mutate
import verify_length_cases as cases  # noqa: F401 (the `case` fixture's catalogues)
from conftest import ROOT
from test_gpu_verify_device import golden, upload
from test_gpu_verify_lengths import MALFORMED, MODES, Report, case, got, rv  # noqa: F401 (case, rv: fixtures)
from test_verify_device_host import expected_table, with_counts

pytestmark = pytest.mark.gpu

NAMES = ("gf2_mix", "z64_mix", "sizehint_mixed", "adder64", "empty", "ref_test")
E_ARG = 9


def lib():
    from reverie_amd import _lib

    return _lib.lib()


def paths():
    """(proofs verified in one pass on the device, by the single-proof device verifier, from a host copy)"""
    out = (C.c_uint64 * 3)()
    assert lib().rv_hook_verify_batch_device_paths(out) == 0
    return tuple(int(x) for x in out)


def moved(before):
    return tuple(a - b for a, b in zip(paths(), before))


def proof_len_of(circuit):
    """the documented length of a proof of the circuit"""
    sz2, sz64 = circuit.record_sizes()
    return 32 + 4 * 8 + 40 * (sz2 + sz64) + 2 * 216 * 48


def statements(rv, circuit, w2, w64, rule_seeds, batch):
    """`batch` statements of the circuit: the golden witness and seeds first, then other seeds and -- where the circuit has inputs
    and the changed witness still satisfies it -- other witnesses"""
    g = np.tile(np.asarray(w2, np.uint8), (batch, 1))
    z = np.tile(np.asarray(w64, np.uint64), (batch, 1))
    seeds = np.stack([np.roll(rule_seeds, b, axis=0) ^ np.uint8(b) for b in range(batch)]).astype(np.uint8)
    for b in range(1, batch):
        gb, zb = g[b].copy(), z[b].copy()
        if gb.size:
            gb[b % gb.size] ^= 1
        if zb.size:
            zb[b % zb.size] += np.uint64(b)
        try:  # (a witness the circuit's assertions refuse stays the golden one)
            rv.Proof.new(circuit, gb, zb, seeds=seeds[b])
            g[b], z[b] = gb, zb
        except rv.ReverieError as e:
            assert e.code == 1, e
    return g, z, seeds


def host_batch(rv, circuit, g, z, seeds):
    return [bytes(p) for p in rv.Proof.new_batch(circuit, g, z if z.shape[1] else None, seeds=seeds)]


def device_batch(rv, circuit, g, z, seeds):
    """the bytes prove_batch_device left, proof by proof"""
    dps = rv.prove_batch_device(circuit, g, z if z.shape[1] else None, seeds=seeds)
    return dps, [dp.tensor.cpu().numpy().tobytes() for dp in dps]


_circuits = {}


@pytest.fixture
def gold(rv, name):
    if name not in _circuits:
        prog, w2, w64, wc, proof = golden(name)
        _circuits[name] = dict(circuit=rv.Circuit(prog, wc), w2=w2, w64=w64, proof=proof)
    return _circuits[name]


# ---- the prover
@pytest.mark.parametrize("batch", (1, 2, 5))
@pytest.mark.parametrize("name", NAMES)
def test_prover_parity(rv, rule_seeds, gold, name, batch):
    c = gold["circuit"]
    g, z, seeds = statements(rv, c, gold["w2"], gold["w64"], rule_seeds, batch)
    dps, have = device_batch(rv, c, g, z, seeds)
    want = host_batch(rv, c, g, z, seeds)
    assert len(have) == batch and all(len(p) == proof_len_of(c) for p in have)
    assert have == want
    assert have[0] == gold["proof"]  # (statement 0: the golden witness and seeds)
    # all of them views of one tensor, a stride of whole 256-byte lines apart
    stride = (proof_len_of(c) + 255) & ~255
    assert [dp.tensor.data_ptr() - dps[0].tensor.data_ptr() for dp in dps] == [b * stride for b in range(batch)]
    assert dps[0].tensor.data_ptr() % 256 == 0


def raw_prove(circuit, g, z, seeds, stride, batch=None, dst=None):
    """rv_prove_batch_device itself -> (code, proof_len, the buffer)"""
    import torch

    batch = g.shape[0] if batch is None else batch
    buf = torch.zeros(max(batch * stride, 256), dtype=torch.uint8, device="cuda") if dst is None else dst
    n = C.c_size_t(0)
    ptr = lambda a: a.ctypes.data_as(C.c_void_p) if a is not None and a.size else None  # noqa: E731
    rc = lib().rv_prove_batch_device(circuit.ctx.handle, circuit.handle, batch, ptr(g), g.shape[1], ptr(z), z.shape[1], ptr(seeds),
                                     C.c_void_p(buf.data_ptr()) if hasattr(buf, "data_ptr") else buf, stride, C.byref(n))
    return rc, n.value, buf


@pytest.mark.parametrize("name", ("z64_mix",))
def test_prover_chunks(rv, rule_seeds, gold, monkeypatch, name):
    c = gold["circuit"]
    g, z, seeds = statements(rv, c, gold["w2"], gold["w64"], rule_seeds, 5)
    _, whole = device_batch(rv, c, g, z, seeds)
    monkeypatch.setenv("RV_BATCH_MAX", "2")
    _, chunked = device_batch(rv, c, g, z, seeds)
    assert chunked == whole and whole[0] == gold["proof"]
    # a stride wider than the proof: every proof at its own place
    stride = ((proof_len_of(c) + 255) & ~255) + 512
    rc, n, buf = raw_prove(c, g, z, seeds, stride)
    assert rc == 0 and n == proof_len_of(c)
    host = buf.cpu().numpy().tobytes()
    assert [host[b * stride:b * stride + n] for b in range(5)] == whole


CHILD = r"""
import ctypes as C, sys
import numpy as np
sys.path[:0] = [{root!r}, {tests!r}]
import reverie_amd as rv
from reverie_amd import _lib
from test_gpu_verify_device import golden, upload
prog, w2, w64, wc, proof = golden("gf2_mix")
c = rv.Circuit(prog, wc)
seeds = np.frombuffer(bytes.fromhex(sys.argv[1]), np.uint8).reshape(2, 256, 16)
g = np.tile(np.asarray(w2, np.uint8), (2, 1))
dps = rv.prove_batch_device(c, g, None, seeds=seeds)
have = [dp.tensor.cpu().numpy().tobytes() for dp in dps]
want = [bytes(rv.Proof.new(c, w2, w64, seeds=seeds[b])) for b in range(2)]
assert have == want and have[0] == proof, "large-circuit branch: bytes differ"
out = (C.c_uint64 * 3)()
bad = bytearray(proof); bad[len(proof) // 2] ^= 1
answers = rv.verify_batch_device(c, dps + [upload(bytes(bad)), upload(proof[:100])])
assert answers == rv.verify_batch(c, have + [bytes(bad), proof[:100]]) == [True, True, False, False], answers
_lib.lib().rv_hook_verify_batch_device_paths(out)
assert tuple(out) == (0, 3, 1), tuple(out)
print("child ok")
"""


def test_large_circuit_branch(rule_seeds):
    """RV_BATCH_BIG_GATES is read once per process: a fresh child in which gf2_mix counts as a large circuit proves two statements
    one after the other (the same bytes) and verifies its proofs through the single-proof device verifier"""
    seeds = np.stack([rule_seeds, rule_seeds[::-1]]).astype(np.uint8)
    env = dict(os.environ, RV_BATCH_BIG_GATES="1")
    code = CHILD.format(root=ROOT, tests=os.path.join(ROOT, "tests"))
    r = subprocess.run([sys.executable, "-c", code, seeds.tobytes().hex()], env=env, cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "child ok" in r.stdout, r.stdout + r.stderr


# ---- the verifier
def altered_that_frames(proof):
    """a catalogue entry with a longer vector in all eight records of a group: it frames, and check_records takes it"""
    for label, data in proof_mutate.catalogue(proof, targets=(("all8", 0),), same_length=False):
        if label.endswith(":+8x00") or label.endswith(":+8xFF"):
            return data
    raise AssertionError("no such entry")


def mixed_batch(proof, second):
    t = expected_table(proof)
    cut = t[8 * 3 + 0] + 50  # inside record 3's keys
    return [proof, altered_that_frames(proof), proof[:cut], second, with_counts(proof, [2], 41)]


def answers_of(fn):
    from reverie_amd import ReverieError

    try:
        return fn()
    except ReverieError as e:
        return ("err", e.code)


def both(rv, circuit, datas, strict):
    """(rv_verify_batch's answer on the bytes, rv_verify_batch_device's on uploaded copies, what the device call's proofs did)"""
    tensors = [upload(d) for d in datas]
    want = answers_of(lambda: rv.verify_batch(circuit, datas, strict=strict))
    before = paths()
    have = answers_of(lambda: rv.verify_batch_device(circuit, tensors, strict=strict))
    return want, have, moved(before)


@pytest.mark.parametrize("name", NAMES)
def test_verifier_equals_host_batch(rv, rule_seeds, gold, name):
    c = gold["circuit"]
    second = bytes(rv.Proof.new(c, gold["w2"], gold["w64"], seeds=rule_seeds[::-1].copy()))
    datas = mixed_batch(gold["proof"], second)
    for strict, _ in MODES:
        want, have, went = both(rv, c, datas, strict)
        assert have == want, (strict, have, want)
        assert want[0] is True and want[3] is True and want[2] is False and want[4] is False
        assert went[0] >= 3 and went[1] == 0 and went[2] == 2 and sum(went) == 5, went


def test_fewer_than_two_live(rv):
    prog, w2, w64, wc, proof = golden("gf2_mix")
    c = rv.Circuit(prog, wc)
    try:
        datas = [proof[:31], proof, proof[:len(proof) - 1]]
        for strict, _ in MODES:
            want, have, went = both(rv, c, datas, strict)
            assert have == want == [False, True, False]
            assert went == (0, 1, 2)
        # a batch of one: the single-proof path whatever the proof
        want, have, went = both(rv, c, [proof], True)
        assert have == want == [True] and went == (0, 1, 0)
    finally:
        c.close()


@pytest.mark.parametrize("name", ("MIX", "Z"))
def test_different_lengths_in_one_batch(rv, case, name):
    """the catalogue's thin axis, the entries the oracle answers with a bool (their lengths are settled by the digests, not by
    the framing): proofs of many lengths in one batch, each beside the unaltered proof"""
    rep = Report(f"{name} rv_verify_batch_device")
    idx = [i for i in case["thin"] if all(a != MALFORMED for a in case["answers"][i])]
    assert len(idx) >= 20
    good = upload(case["good"])
    tensors = {i: upload(case["entries"][i][1]) for i in idx}
    assert len({len(case["entries"][i][1]) for i in idx}) >= 5
    for at in range(0, len(idx), 24):
        part = idx[at:at + 24]
        datas, proofs = [case["good"]], [good]
        for i in part:
            datas += [case["entries"][i][1], case["good"]]
            proofs += [tensors[i], good]
        for strict, k in MODES:
            before = paths()
            have = rv.verify_batch_device(case["circuit"], proofs, strict=strict)
            assert moved(before) == (len(proofs), 0, 0)
            assert have == rv.verify_batch(case["circuit"], datas, strict=strict)
            assert all(have[0::2])
            for j, i in enumerate(part):
                rep.check(case["entries"][i][0], f"strict={strict}", have[2 * j + 1], case["answers"][i][k])
    rep.done()


@pytest.mark.parametrize("name", ("z64_mix", "gf2_mix"))
def test_verifier_chunks(rv, rule_seeds, gold, monkeypatch, name):
    c = gold["circuit"]
    second = bytes(rv.Proof.new(c, gold["w2"], gold["w64"], seeds=rule_seeds[::-1].copy()))
    datas = mixed_batch(gold["proof"], second)
    whole = both(rv, c, datas, True)
    monkeypatch.setenv("RV_BATCH_MAX", "2")
    want, have, went = both(rv, c, datas, True)
    assert have == want == whole[0] == whole[1]
    # chunks of (2, 2, 1) proofs: [good, altered] in one pass, [cut, good] and [wrong count] proof after proof
    assert went == (2, 1, 2), went


@pytest.mark.parametrize("name", ("adder64",))
def test_round_trip_in_device_memory(rv, rule_seeds, gold, name):
    c = gold["circuit"]
    g, z, seeds = statements(rv, c, gold["w2"], gold["w64"], rule_seeds, 4)
    dps = rv.prove_batch_device(c, g, z if z.shape[1] else None, seeds=seeds)
    uploaded = lib().rv_hook_verify_proof_bytes()  # (the host verifiers' host-to-device proof bytes)
    before = paths()
    assert rv.verify_batch_device(c, dps) == [True] * 4
    assert rv.verify_batch_device(c, dps, strict=False) == [True] * 4
    t = expected_table(dps[1].tensor.cpu().numpy().tobytes())
    assert t[4] > 0  # (record 0 of the GF(2) domain has a corrections vector)
    dps[1].tensor[t[3]] ^= 0x80
    assert rv.verify_batch_device(c, dps) == [True, False, True, True]
    assert moved(before) == (12, 0, 0)
    assert lib().rv_hook_verify_proof_bytes() == uploaded, "proofs verified in device memory were uploaded"
    assert rv.prove_batch_device(c, g[:0], None) == [] and rv.verify_batch_device(c, []) == []
    # seeds from the OS
    assert rv.verify_batch_device(c, rv.prove_batch_device(c, g[:2], z[:2] if z.shape[1] else None)) == [True, True]


def test_argument_errors(rv, rule_seeds):
    import torch

    prog, w2, w64, wc, proof = golden("gf2_mix")
    c = rv.Circuit(prog, wc)
    L = lib()
    try:
        n = proof_len_of(c)
        assert n == len(proof)
        stride = (n + 255) & ~255
        g = np.tile(np.asarray(w2, np.uint8), (2, 1))
        z = np.zeros((2, 0), np.uint64)
        seeds = np.stack([rule_seeds, rule_seeds]).astype(np.uint8)
        before = paths()
        # ---- the prover: stride, seeds, the buffer
        poison = lambda: torch.full((2 * stride + 512,), 0xA5, dtype=torch.uint8, device="cuda")  # noqa: E731
        for bad_stride in (stride + 128, stride + 8, stride - 256, 0):
            buf = poison()
            rc, got_n, _ = raw_prove(c, g, z, seeds, bad_stride, dst=buf)
            assert rc == E_ARG and got_n == n, bad_stride
            assert bool((buf == 0xA5).all()), "a refused call wrote into the buffer"
        buf = poison()
        assert raw_prove(c, g, z, None, stride, dst=buf)[0] == E_ARG  # seeds == NULL
        assert raw_prove(c, g, z, seeds, stride, dst=buf[16:])[0] == E_ARG  # not 256-byte aligned
        small = torch.full((stride,), 0xA5, dtype=torch.uint8, device="cuda")
        host = np.zeros(2 * stride + 256, np.uint8)
        host_at = (host.ctypes.data + 255) & ~255
        assert raw_prove(c, g, z, seeds, stride, dst=C.c_void_p(host_at))[0] == E_ARG  # host memory
        assert raw_prove(c, g, z, seeds, stride, dst=None, batch=0)[0] == E_ARG
        # past the allocation (torch's caching allocator hands out blocks of at least 512 bytes: a batch far beyond the block)
        assert raw_prove(c, np.tile(g, (4096, 1)), np.zeros((8192, 0), np.uint64), np.tile(seeds, (4096, 1, 1)), stride, dst=small)[0] == E_ARG
        assert bool((small == 0xA5).all()) and bool((buf == 0xA5).all())
        # ---- the verifier
        t = upload(proof)
        shifted = upload(bytes(8) + proof)[8:]
        ok = (C.c_int * 2)(7, 7)

        def call(ptrs, lens, flags=0, ok=ok):
            return L.rv_verify_batch_device(c.ctx.handle, c.handle, len(ptrs), (C.c_void_p * len(ptrs))(*ptrs), (C.c_size_t * len(lens))(*lens), flags, ok)

        hostp = np.frombuffer(proof, np.uint8).copy()
        assert call([t.data_ptr(), hostp.ctypes.data], [n, n]) == E_ARG  # a host pointer
        assert call([t.data_ptr(), shifted.data_ptr()], [n, n]) == E_ARG  # misaligned by 8
        assert call([t.data_ptr(), t.data_ptr()], [n, 1 << 40]) == E_ARG  # a length past the allocation
        assert call([t.data_ptr(), None], [n, n]) == E_ARG
        for flags in (3, 4, 1 << 31):  # both bits, unknown bits
            assert call([t.data_ptr(), t.data_ptr()], [n, n], flags) == E_ARG
        assert call([t.data_ptr(), t.data_ptr()], [n, n], 0, None) == E_ARG
        assert L.rv_verify_batch_device(c.ctx.handle, c.handle, 0, None, None, 0, ok) == E_ARG
        assert paths() == before
        assert call([t.data_ptr(), t.data_ptr()], [n, n]) == 0 and list(ok) == [1, 1]
        assert moved(before) == (2, 0, 0)
        # ---- Python: what is refused before the library is called
        with pytest.raises(TypeError):
            rv.verify_batch_device(c, [proof])
        with pytest.raises(TypeError):
            rv.verify_batch_device(c, [t.cpu()])
        with pytest.raises(TypeError):
            rv.verify_batch_device(c, [rv.DeviceProof.new(c, w2, w64, seeds=rule_seeds)])
        with pytest.raises(ValueError):
            rv.verify_batch_device(c, [t.view(2, -1)])
        with pytest.raises(TypeError):
            rv.verify_batch_device(prog, [t])
        with pytest.raises(TypeError):
            rv.prove_batch_device(prog, g)
        assert moved(before) == (2, 0, 0)
    finally:
        c.close()
