"""rv_verify_device / rv_verify_sections_device, the part that needs no GPU: the symbols, and the framing walk (walk_proof,
reverie_amd/csrc/verify_dev.h -- the function k_parse_proof runs on the device) against tests/proof_mutate.parse.

The walk decides which calls take the device path, and it is the only code that reads a hostile byte string on the GPU, so:
every committed golden proof (table and status), every prefix of proof_empty.bin, the four repetition counts set to 0, 39, 41
and 2^63, check_records' rules, the sections framing -- and the same walks in a stand-alone program built with
-fsanitize=address,undefined, where every input is a heap block of exactly its length."""
import ctypes as C
import glob
import os
import re
import struct
import subprocess

import numpy as np
import pytest

import proof_mutate
from conftest import GOLDEN, ROOT

WORDS, REC, PRE, STATUS, OMIT, COMM = 657, 0, 640, 642, 643, 653  # csrc/verify_dev.h: the table's layout
OK, SHORT, COUNT, SECTION, RECORDS = 0, 1, 2, 3, 4
GOLDEN_PROOFS = sorted(glob.glob(os.path.join(GOLDEN, "proof_*.bin")))


@pytest.fixture(scope="module")
def L():
    from reverie_amd import _lib

    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__

        __graft_entry__.build()
    return _lib.lib()


def walk(L, data: bytes, framing=0, lens=None):
    """-> (status, table as a list of 657 ints)"""
    table = (C.c_uint64 * WORDS)()
    if lens is not None:
        table[0:4] = lens
    status = C.c_int(-1)
    buf = (C.c_uint8 * max(len(data), 1)).from_buffer_copy(data or b"\0")
    assert L.rv_hook_verify_walk(buf, len(data), framing, table, C.byref(status)) == 0
    assert table[STATUS] == status.value
    return status.value, list(table)


def expected_table(proof: bytes):
    """the table of a proof proof_mutate.parse takes apart"""
    comm, domains = proof_mutate.parse(proof)
    t = [0] * WORDS
    omit = bytearray(80)
    pos = 32
    for d, (records, pre) in enumerate(domains):
        assert len(records) == 40 and len(pre) == 216 * 48
        pos += 8
        for i, (om, keys, vecs) in enumerate(records):
            k = 40 * d + i
            omit[k] = om
            t[8 * k + 7] = om
            t[8 * k + 0] = pos + 1
            pos += 129
            for v, vec in enumerate(vecs):
                pos += 8
                t[8 * k + 1 + 2 * v], t[8 * k + 2 + 2 * v] = pos, len(vec)
                pos += len(vec)
        pos += 8
        t[PRE + d] = pos
        pos += len(pre)
    assert pos == len(proof)
    t[OMIT:OMIT + 10] = struct.unpack("<10Q", bytes(omit))
    t[COMM:COMM + 4] = struct.unpack("<4Q", comm)
    return t


def sections_of(proof: bytes):
    """-> (the four sections joined, lens[4]) of a proof that parses"""
    t = expected_table(proof)
    parts = []
    for d in range(2):
        on0, pre0 = t[8 * 40 * d] - 1, t[PRE + d]
        parts += [proof[on0:pre0 - 8], proof[pre0:pre0 + 216 * 48]]
    return b"".join(parts), [len(p) for p in parts]


def with_counts(proof: bytes, which, value):
    t = expected_table(proof)
    at = [32, t[PRE] - 8, t[PRE] + 216 * 48, t[PRE + 1] - 8]
    out = bytearray(proof)
    for i in which:
        out[at[i]:at[i] + 8] = struct.pack("<Q", value)
    return bytes(out)


def test_symbols_exported_and_bound(L):
    import reverie_amd
    from reverie_amd import _lib

    hdr = open(os.path.join(ROOT, "include", "reverie_amd.h")).read()
    for name in ("rv_verify_device", "rv_verify_sections_device", "rv_hook_verify_device_paths", "rv_hook_verify_walk", "rv_hook_verify_schedule"):
        assert name in _lib.SYMBOLS and name in _lib.ARGTYPES
        assert getattr(L, name).argtypes is not None and getattr(L, name).restype is C.c_int
        assert re.search(r"\b" + name + r"\s*\(", hdr), name
    assert L.rv_abi_version() == 8
    assert reverie_amd.DeviceProof is reverie_amd.proof.DeviceProof
    paths = (C.c_uint64 * 2)()
    assert L.rv_hook_verify_device_paths(paths) == 0 and L.rv_hook_verify_device_paths(None) == 9
    assert L.rv_hook_verify_schedule((C.c_uint64 * 8)()) == 0 and L.rv_hook_verify_schedule(None) == 9


def test_hook_arguments(L):
    table = (C.c_uint64 * WORDS)()
    status = C.c_int()
    buf = (C.c_uint8 * 64)()
    assert L.rv_hook_verify_walk(buf, 64, 2, table, C.byref(status)) == 9  # an unknown framing
    assert L.rv_hook_verify_walk(None, 64, 0, table, C.byref(status)) == 9
    assert L.rv_hook_verify_walk(buf, 64, 0, None, C.byref(status)) == 9
    table[0:4] = [16, 16, 16, 17]  # sections that do not add up to the length
    assert L.rv_hook_verify_walk(buf, 64, 1, table, C.byref(status)) == 9
    table[0:4] = [1 << 63, 1 << 63, 16, 16]  # ... or whose sum wraps
    assert L.rv_hook_verify_walk(buf, 32, 1, table, C.byref(status)) == 9


@pytest.mark.parametrize("path", GOLDEN_PROOFS, ids=os.path.basename)
def test_walk_golden(L, path):
    proof = open(path, "rb").read()
    want = expected_table(proof)
    status, table = walk(L, proof)
    assert status == OK and table == want
    for tail in (b"\0", b"\xff" * 4096):  # bytes behind the proof are ignored
        status, table = walk(L, proof + tail)
        assert status == OK and table == want
    # the same records as sections: 40 bytes nearer the front in the first domain (comm, one count), 56 in the second
    sec, lens = sections_of(proof)
    status, table = walk(L, sec, 1, lens)
    assert status == OK
    for k in range(80):
        shift = 40 if k < 40 else 56
        assert table[8 * k:8 * k + 8] == [w - (shift if j in (0, 1, 3, 5) else 0) for j, w in enumerate(want[8 * k:8 * k + 8])]
    assert table[PRE] == want[PRE] - 48 and table[PRE + 1] == want[PRE + 1] - 64
    assert table[OMIT:OMIT + 10] == want[OMIT:OMIT + 10] and table[COMM:COMM + 4] == [0] * 4
    # a section that does not end where its records do, a preprocessing section of another size
    for i in range(4):
        for delta in (-1, 1):
            l2 = list(lens)
            l2[i] += delta
            s2 = sec[:sum(l2)].ljust(sum(l2), b"\0")
            assert walk(L, s2, 1, l2)[0] in (SECTION, SHORT), (i, delta)
    assert walk(L, sec + b"\0", 1, [lens[0], lens[1], lens[2] + 1, lens[3]])[0] == SECTION


def test_walk_every_truncation(L):
    proof = open(os.path.join(GOLDEN, "proof_empty.bin"), "rb").read()
    assert walk(L, proof)[0] == OK
    table = (C.c_uint64 * WORDS)()
    status = C.c_int()
    buf = (C.c_uint8 * len(proof)).from_buffer_copy(proof)
    for n in range(len(proof)):
        assert L.rv_hook_verify_walk(buf, n, 0, table, C.byref(status)) == 0
        assert status.value == SHORT, n
    for n in (0, 31, 32, 39, 40, 41, 169, 170, len(proof) - 1):  # ... which is what the parser says of them
        with pytest.raises((ValueError, struct.error)):
            proof_mutate.parse(proof[:n])


@pytest.mark.parametrize("value", [0, 39, 41, 1 << 63])
def test_walk_counts(L, value):
    for path in GOLDEN_PROOFS:
        proof = open(path, "rb").read()
        for which in ([0], [1], [2], [3], [0, 1, 2, 3]):
            assert walk(L, with_counts(proof, which, value))[0] == COUNT, (path, which)


def test_walk_record_rules(L):
    """check_records (csrc/verify.inc): omit >= 8 in either domain; within a GF(2) group rec lengths equal, corr and in not
    below the group's first -- Z64 lengths are free"""
    proof = open(os.path.join(GOLDEN, "proof_gf2_mix.bin"), "rb").read()
    comm, good = proof_mutate.parse(proof)

    def status(change):
        doms = proof_mutate._copy(good)
        change(doms)
        data = proof_mutate.serialise(comm, doms)
        st, table = walk(L, data)
        if st == OK:
            assert table == expected_table(data)
        return st

    def set_omit(d, r, v):
        return lambda doms: doms[d][0][r].__setitem__(0, v)

    def resize(d, r, v, delta):
        def change(doms):
            old = doms[d][0][r][2][v]
            doms[d][0][r][2][v] = old[:len(old) + delta] if delta < 0 else old + b"\xff" * delta
        return change

    assert len(good[0][0][0][2][1]) > 0 and len(good[0][0][0][2][2]) > 0
    for d in (0, 1):
        assert status(set_omit(d, 39, 8)) == RECORDS and status(set_omit(d, 0, 255)) == RECORDS
        assert status(set_omit(d, 17, 7)) == OK
    for r in (3, 39):
        assert status(resize(0, r, 0, 1)) == RECORDS and status(resize(0, r, 0, -1)) == RECORDS  # rec: equal
        for v in (1, 2):  # corr, in: not below the first record's
            assert status(resize(0, r, v, -1)) == RECORDS and status(resize(0, r, v, 3)) == OK
    assert status(resize(0, 8, 1, -1)) == OK  # (a group's first record sets the length)
    for v in range(3):
        assert status(resize(1, 3, v, 9)) == OK and status(resize(1, 0, v, 1)) == OK


def test_walk_under_sanitizers(L, tmp_path):
    """the stand-alone program (tests/verify_walk_asan.cpp): clean under AddressSanitizer and UBSan, and walk for walk the
    library's answers"""
    exe = str(tmp_path / "verify_walk_asan")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", os.path.join(ROOT, "reverie_amd", "csrc"), os.path.join(ROOT, "tests", "verify_walk_asan.cpp"), "-o", exe])
    empty = os.path.join(GOLDEN, "proof_empty.bin")
    others = [p for p in GOLDEN_PROOFS if p != empty]
    run = subprocess.run([exe] + others + ["--prefixes", empty], capture_output=True, text=True)
    assert run.returncode == 0 and "Sanitizer" not in run.stderr and "runtime error" not in run.stderr, run.stderr[-2000:]
    lines = run.stdout.split("\n")
    assert lines[-2] == "bad 0" and f"prefixes {os.path.getsize(empty)}" in lines

    def fnv(table):
        h = 0xCBF29CE484222325
        for b in np.asarray(table, np.uint64).tobytes():
            h = ((h ^ b) * 0x100000001B3) & ((1 << 64) - 1)
        return h

    whole = [ln.split() for ln in lines if ln.startswith(("proof ", "sections "))]
    assert len(whole) == 2 * len(GOLDEN_PROOFS)
    for path, (a, b) in zip(others + [empty], zip(whole[0::2], whole[1::2])):
        proof = open(path, "rb").read()
        sec, lens = sections_of(proof)
        for (what, n, status, h), (data, framing, ls) in zip((a, b), ((proof, 0, None), (sec, 1, lens))):
            st, table = walk(L, data, framing, ls)
            assert (int(n), int(status), int(h, 16)) == (len(data), st, fnv(table)), (path, what)
    counts = [ln.split() for ln in lines if ln.startswith("count ")]
    assert len(counts) == 16 and all(int(c[2]) == COUNT for c in counts)


def test_device_proof_refuses_host_tensors():
    """before any library call: no context is made (there is no GPU here to make one on)"""
    import torch

    import reverie_amd

    with pytest.raises(TypeError):
        reverie_amd.DeviceProof(torch.zeros(64, dtype=torch.uint8))
    with pytest.raises(TypeError):
        reverie_amd.DeviceProof(np.zeros(64, np.uint8))
    with pytest.raises(TypeError):
        reverie_amd.DeviceProof(sections=torch.zeros(64, dtype=torch.uint8), lens=[16, 16, 16, 16], comm=bytes(32))
    with pytest.raises(ValueError):
        reverie_amd.DeviceProof()
    with pytest.raises(ValueError):
        reverie_amd.DeviceProof(sections=torch.zeros(64, dtype=torch.uint8), lens=[64], comm=bytes(32))
