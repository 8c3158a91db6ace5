"""Run by tests/test_gpu_verify_multirank.py in a FRESH process with RV_RCCL_PATH = the rccl test shim (tests/rccl_shim): the
library's multi-rank verifier -- rv_comm_create_all + rv_verify_multi (a host thread per rank, rv_verify_sharded on each: its
groups of the partition, one all-gather of slot digests, the decision on every rank; csrc/comm.inc) -- with 2, 4 and 8 ranks that
share the one GPU.  Every (rc, ok) must be rv_verify_ex's.  Prints one JSON line."""
import ctypes as C
import json
import os
import struct
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402

import circuits  # noqa: E402
import reverie_amd  # noqa: E402
from conftest import GOLDEN, golden_ops  # noqa: E402
from reverie_amd import _lib  # noqa: E402
from reverie_amd.ops import program  # noqa: E402

COMPAT = 2


def rule_seeds():
    import oracle_lib

    oracle_lib.build()
    seeds = np.zeros((256, 16), np.uint8)  # seed[r] = BLAKE3("rv-seed" || LE32(r))[0..16] (tests/conftest.py: rule_seeds)
    buf = C.create_string_buffer(32)
    for r in range(256):
        d = b"rv-seed" + struct.pack("<I", r)
        oracle_lib.lib().rvo_blake3_hash(d, C.c_size_t(len(d)), buf)
        seeds[r] = np.frombuffer(buf.raw[:16], np.uint8)
    return seeds


def broadcast_offset(proof: bytes, record: int) -> int:
    """offset of the first byte of the broadcast vector of GF(2) online record `record` (slot `record`)"""
    u64 = lambda at: struct.unpack_from("<Q", proof, at)[0]  # noqa: E731
    pos = 32 + 8
    for i in range(40):
        pos += 1 + 128
        n_rec = u64(pos)
        pos += 8
        if i == record:
            assert n_rec > 0
            return pos
        pos += n_rec
        pos += 8 + u64(pos)
        pos += 8 + u64(pos)
    raise AssertionError


def flip(proof: bytes, at: int) -> bytes:
    b = bytearray(proof)
    b[at] ^= 0xFF
    return bytes(b)


def verify_ex(circ, proof: bytes, flags):
    ok = C.c_int()
    buf = (C.c_uint8 * len(proof)).from_buffer_copy(proof)
    rc = _lib.lib().rv_verify_ex(circ.ctx.handle, circ.handle, buf, C.c_size_t(len(proof)), C.c_uint32(flags), C.byref(ok))
    return rc, ok.value


def main():
    assert os.environ.get("RV_RCCL_PATH"), "the worker must run against the shim"
    L = _lib.lib()
    seeds = rule_seeds()
    full = bool(os.environ.get("MULTI_FULL"))
    # (name, program, wire counts, proof, the (rc, ok) wanted strict and in compatibility mode)
    cases = []
    if full:
        # BASELINE config 4 at full size: the 50 MB proof of rv_prove, and the same with the last online record's broadcast vector
        # touched (online group 4)
        prog, wit, wc, _ = circuits.layered_gf2()
        proof = bytes(reverie_amd.Proof.new(prog, wit, [], wc, seeds=seeds))
        cases.append(("config4", prog, wc, proof, ((0, 1), (0, 1))))
        cases.append(("config4-flipped", prog, wc, flip(proof, broadcast_offset(proof, 39)), ((0, 0), (0, 0))))
    else:
        rng = np.random.default_rng(77)
        prog, w2, w64, wc = circuits.random_mixed(rng, n_gates=400)
        proof = bytes(reverie_amd.Proof.new(prog, w2, w64, wc, seeds=seeds))
        cases.append(("mixed", prog, wc, proof, ((0, 1), (0, 1))))
        # online group 1 (slots 8..15): rank 1 of the partition, never rank 0
        cases.append(("mixed-flipped", prog, wc, flip(proof, broadcast_offset(proof, 12)), ((0, 0), (0, 0))))
        cases.append(("mixed-truncated", prog, wc, proof[:len(proof) // 2], ((4, 0), (4, 0))))
        prog, wit, wc, _ = circuits.layered_gf2(n_in=300, width=4096, layers=6)
        cases.append(("layered", prog, wc, bytes(reverie_amd.Proof.new(prog, wit, [], wc, seeds=seeds)), ((0, 1), (0, 1))))
        cm1, cm2, w2, w64, wcm = circuits.assert_circuits()
        cases.append(("false-statement", cm2, wcm, bytes(reverie_amd.Proof.new(cm1, w2, w64, wcm, seeds=seeds)), ((0, 0), (0, 1))))
        cases.append(("forged-omit",) + forged_omit(seeds) + (((0, 0), (0, 1)),))
    worlds = [int(x) for x in (sys.argv[1:] or ["2", "4", "8"])]
    res = {}
    for n in worlds:
        ctxs = [reverie_amd.Context(0) for _ in range(n)]
        hc = (C.c_void_p * n)(*[cx.handle for cx in ctxs])
        cm = (C.c_void_p * n)()
        _lib.check(L.rv_comm_create_all(hc, C.c_int(n), cm))
        compiled = {}  # one circuit per program and rank
        for name, prog, wc, proof, want in cases:
            if id(prog) not in compiled:
                compiled[id(prog)] = [reverie_amd.Circuit(prog, wc, cx) for cx in ctxs]
            circs = compiled[id(prog)]
            hcirc = (C.c_void_p * n)(*[c.handle for c in circs])
            buf = (C.c_uint8 * len(proof)).from_buffer_copy(proof)
            for flags, w in zip((0, COMPAT), want):
                ok = C.c_int(-1)
                t0 = time.perf_counter()
                rc = L.rv_verify_multi(cm, hcirc, C.c_int(n), buf, C.c_size_t(len(proof)), C.c_uint32(flags), C.byref(ok))
                dt = time.perf_counter() - t0
                got = (rc, ok.value)
                single = verify_ex(circs[0], proof, flags)
                res["%s/%d/%s" % (name, n, "strict" if flags == 0 else "compat")] = got == w == single and (rc == 0 or dt < 10.0)
                if got != w or got != single:
                    print("MISMATCH", name, n, flags, got, w, single, L.rv_last_error().decode(), file=sys.stderr)
        for circs in compiled.values():
            for c in circs:
                c.close()
        for i in range(n):
            L.rv_comm_destroy(C.c_void_p(cm[i]))
        for cx in ctxs:
            cx.close()
    print(json.dumps(res))
    return 0 if all(res.values()) else 1


def forged_omit(seeds):
    """a proof whose records hide another player than the challenge names (test_strict_verify_omit_must_match_challenge)"""
    from reverie_amd.dist import HipShardBackend, assemble
    from reverie_amd.proof import challenge, combine_digests

    m = json.load(open(os.path.join(GOLDEN, "proofs.json")))["adder64"]
    prog = program(golden_ops(m))
    wc = tuple(m["wire_counts"])
    c = reverie_amd.Circuit(prog, wc)
    be = HipShardBackend(c)
    shard = be.commit(m["wit_gf2"], [int(x) for x in m["wit_z64"]], seeds, 0, 256)
    try:
        comm = combine_digests(be.digests(shard))
        omit = challenge(comm)
        k = int(np.flatnonzero(omit < 8)[7])
        omit[k] = (omit[k] + 3) % 8
        blob, lens, _, _ = be.open(shard, omit)
    finally:
        be.destroy(shard)
    c.close()
    return prog, wc, assemble(comm, [(blob, lens)])


if __name__ == "__main__":
    sys.exit(main())
