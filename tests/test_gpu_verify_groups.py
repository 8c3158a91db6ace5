"""rv_verify_shard_groups on one GPU: the verifier's 32 groups of eight slots split over the ranks of a world (the partition
rv_verify_sharded uses, and the contiguous split), every rank's groups verified one after the other on one context, the
digests placed by slot and decided by rv_verify_finish_ex.  The answer must be rv_verify_ex's and the oracle's, strict and in
compatibility mode; a shard must copy exactly its online groups' records to the device (rv_hook_verify_proof_bytes)."""
import ctypes as C
import json
import os
import struct

import numpy as np
import pytest

import circuits
from conftest import GOLDEN, golden_matches, golden_ops
from reverie_amd.ops import OP_DTYPE, program

pytestmark = pytest.mark.gpu

META = json.load(open(os.path.join(GOLDEN, "proofs.json")))
WORLDS = [2, 4, 8]
RV_E_ARG = 9
COMPAT = 2


@pytest.fixture(scope="module")
def rv():
    import reverie_amd

    reverie_amd.Context.default()
    return reverie_amd


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def parse_records(proof: bytes):
    """[domain][record] -> (first byte, length, broadcast vector offset, its length) of the 40 online records of both domains"""
    u64 = lambda at: struct.unpack_from("<Q", proof, at)[0]  # noqa: E731
    pos, out = 32, []
    for _ in range(2):
        n, pos = u64(pos), pos + 8
        recs = []
        for _ in range(n):
            start = pos
            pos += 1 + 128
            n_rec, pos = u64(pos), pos + 8
            rec = pos
            pos += n_rec
            pos += 8 + u64(pos)
            pos += 8 + u64(pos)
            recs.append((start, pos - start, rec, n_rec))
        pos += 8 + 48 * u64(pos)
        out.append(recs)
    return out


def span_bytes(proof: bytes, groups) -> int:
    recs = parse_records(proof)
    return sum(recs[d][r][1] for d in range(2) for g in groups if g < 5 for r in range(8 * g, 8 * g + 8))


def lists(kind, world):
    from reverie_amd.dist import verify_partition

    if kind == "partition":
        return [verify_partition(world, r) for r in range(world)]
    n = 32 // world
    return [list(range(r * n, (r + 1) * n)) for r in range(world)]


def verify_split(c, proof: bytes, groups_per_rank):
    """-> (256 x 32 slot digests, AND of the zero-check flags, every rank's digests); checks every rank's upload"""
    from reverie_amd import _lib
    from reverie_amd.dist import HipShardBackend

    L = _lib.lib()
    be = HipShardBackend(c)
    dig = np.zeros((256, 32), np.uint8)
    zc, parts = True, []
    for groups in groups_per_rank:
        before = L.rv_hook_verify_proof_bytes()
        d, z = be.verify_groups(proof, groups)
        assert L.rv_hook_verify_proof_bytes() - before == span_bytes(proof, groups), groups
        for k, g in enumerate(groups):
            dig[8 * g:8 * g + 8] = d[8 * k:8 * k + 8]
        zc = zc and z
        parts.append(d)
    return dig, zc, parts


def finish(proof: bytes, dig, flags, zc) -> bool:
    from reverie_amd import _lib

    ok = C.c_int()
    buf = (C.c_uint8 * len(proof)).from_buffer_copy(proof)
    _lib.check(_lib.lib().rv_verify_finish_ex(buf, C.c_size_t(len(proof)), _p(dig), C.c_uint32(flags), C.c_int(int(zc)), C.byref(ok)))
    return bool(ok.value)


def verify_ex(c, proof: bytes, flags) -> bool:
    from reverie_amd import _lib

    ok = C.c_int()
    buf = (C.c_uint8 * len(proof)).from_buffer_copy(proof)
    _lib.check(_lib.lib().rv_verify_ex(c.ctx.handle, c.handle, buf, C.c_size_t(len(proof)), C.c_uint32(flags), C.byref(ok)))
    return bool(ok.value)


def check_all_splits(rv, oracle, prog, wc, proof: bytes, want=None):
    """every world, both kinds of split, strict and compat: the split answer == rv_verify_ex == the oracle (== want)"""
    c = rv.Circuit(prog, wc)
    answers = {f: verify_ex(c, proof, f) for f in (0, COMPAT)}
    assert answers == {f: oracle.verify(prog, wc, proof, strict=f == 0) for f in (0, COMPAT)}
    if want is not None:
        assert (answers[0], answers[COMPAT]) == want
    for world in WORLDS:
        for kind in ("partition", "contiguous"):
            dig, zc, _ = verify_split(c, proof, lists(kind, world))
            for f in (0, COMPAT):
                assert finish(proof, dig, f, zc) == answers[f], (world, kind, f)
    return answers


@pytest.mark.parametrize("name", sorted(META))
def test_golden_proofs_split_over_groups(rv, oracle, rule_seeds, name):
    m = META[name]
    ops = golden_ops(m)
    prog = program(ops) if ops else np.zeros(0, OP_DTYPE)
    wc = tuple(m["wire_counts"])
    if m.get("digest_only"):
        proof = bytes(rv.Proof.new(prog, m["wit_gf2"], [int(x) for x in m["wit_z64"]], wc, seeds=rule_seeds))
        assert golden_matches(oracle, name, m, proof)
    else:
        proof = open(os.path.join(GOLDEN, f"proof_{name}.bin"), "rb").read()
    check_all_splits(rv, oracle, prog, wc, proof, want=(True, True))


def test_random_mixed_and_z64_heavy(rv, oracle, rule_seeds):
    rng = np.random.default_rng(2024)
    prog, w2, w64, wc = circuits.random_mixed(rng, n_gates=400)
    proof = bytes(rv.Proof.new(prog, w2, w64, wc, seeds=rule_seeds))
    check_all_splits(rv, oracle, prog, wc, proof, want=(True, True))
    prog, wit, wc, _ = circuits.layered_z64(n_in=256, width=2048, n_mul=8000, fold_to=16)
    proof = bytes(rv.Proof.new(prog, [], wit, wc, seeds=rule_seeds))
    check_all_splits(rv, oracle, prog, wc, proof, want=(True, True))


def test_false_statement_and_forged_omit(rv, oracle, rule_seeds):
    from reverie_amd.dist import HipShardBackend, assemble
    from reverie_amd.proof import challenge, combine_digests

    cm1, cm2, w2, w64, wcm = circuits.assert_circuits()
    pm = bytes(rv.Proof.new(cm1, w2, w64, wcm, seeds=rule_seeds))
    check_all_splits(rv, oracle, cm2, wcm, pm, want=(False, True))
    # records that hide another player than the challenge names (test_strict_verify_omit_must_match_challenge)
    m = META["adder64"]
    prog = program(golden_ops(m))
    wc = tuple(m["wire_counts"])
    c = rv.Circuit(prog, wc)
    be = HipShardBackend(c)
    shard = be.commit(m["wit_gf2"], [int(x) for x in m["wit_z64"]], rule_seeds, 0, 256)
    try:
        comm = combine_digests(be.digests(shard))
        omit = challenge(comm)
        forged_omit = omit.copy()
        k = int(np.flatnonzero(omit < 8)[7])
        forged_omit[k] = (omit[k] + 3) % 8
        blob, lens, _, _ = be.open(shard, forged_omit)
        forged = assemble(comm, [(blob, lens)])
    finally:
        be.destroy(shard)
    check_all_splits(rv, oracle, prog, wc, forged, want=(False, True))


def test_flipped_broadcast_byte_only_changes_its_group(rv, oracle, rule_seeds):
    rng = np.random.default_rng(5)
    prog, w2, w64, wc = circuits.random_mixed(rng, n_gates=400)
    honest = bytes(rv.Proof.new(prog, w2, w64, wc, seeds=rule_seeds))
    start, _, rec, n_rec = parse_records(honest)[0][27]  # GF(2) record 27: online group 3
    assert n_rec > 0
    bad = bytearray(honest)
    bad[rec] ^= 0xFF
    bad = bytes(bad)
    check_all_splits(rv, oracle, prog, wc, bad, want=(False, False))
    c = rv.Circuit(prog, wc)
    for world in WORLDS:
        for kind in ("partition", "contiguous"):
            ranks = lists(kind, world)
            _, _, good = verify_split(c, honest, ranks)
            _, _, flip = verify_split(c, bad, ranks)
            changed = [r for r in range(world) if not np.array_equal(good[r], flip[r])]
            assert changed == [next(r for r, g in enumerate(ranks) if 3 in g)], (world, kind)


def test_uploads_and_argument_errors(rv, oracle, rule_seeds):
    from reverie_amd import _lib
    from reverie_amd.dist import HipShardBackend

    L = _lib.lib()
    rng = np.random.default_rng(9)
    prog, w2, w64, wc = circuits.random_mixed(rng, n_gates=300)
    proof = bytes(rv.Proof.new(prog, w2, w64, wc, seeds=rule_seeds))
    c = rv.Circuit(prog, wc)
    be = HipShardBackend(c)
    recs = parse_records(proof)
    online_bytes = sum(r[1] for d in range(2) for r in recs[d])
    assert 0 < online_bytes < len(proof)
    # no online group: no proof bytes
    before = L.rv_hook_verify_proof_bytes()
    be.verify_groups(proof, [31, 5, 17])
    assert L.rv_hook_verify_proof_bytes() == before
    # online groups: exactly their records' spans, both domains, whatever the order
    for groups in ([3], [4, 0], [1, 2, 3], [2, 30, 0]):
        before = L.rv_hook_verify_proof_bytes()
        be.verify_groups(proof, groups)
        assert L.rv_hook_verify_proof_bytes() - before == span_bytes(proof, groups), groups
    # a whole proof (rv_verify = the range form over every group): the 40 online records of both domains, not proof_len
    before = L.rv_hook_verify_proof_bytes()
    assert rv.Proof(proof).verify(c)
    assert L.rv_hook_verify_proof_bytes() - before == online_bytes == span_bytes(proof, range(32))
    # the group order changes nothing but the digests' order
    a, za = be.verify_groups(proof, list(range(32)))
    b, zb = be.verify_groups(proof, list(range(31, -1, -1)))
    assert za and zb and np.array_equal(a.reshape(32, 8, 32)[::-1], b.reshape(32, 8, 32))
    # argument errors
    buf = (C.c_uint8 * len(proof)).from_buffer_copy(proof)
    out = np.zeros((256, 32), np.uint8)
    zc = C.c_int()

    def call(groups, n=None, ctx=c.ctx.handle, pbuf=buf, dig=out):
        g = np.asarray(groups, np.uint8)
        gp = _p(g) if len(g) else None
        return L.rv_verify_shard_groups(ctx, c.handle, pbuf, C.c_size_t(len(proof)), gp, C.c_uint32(len(g) if n is None else n),
                                        None if dig is None else _p(dig), C.byref(zc))

    assert call([0, 5]) == 0
    assert call([0, 0]) == RV_E_ARG
    assert call([5, 6, 5]) == RV_E_ARG
    assert call([32]) == RV_E_ARG
    assert call([255]) == RV_E_ARG
    assert call([0], n=0) == RV_E_ARG
    assert call([]) == RV_E_ARG
    assert call([0], ctx=None) == RV_E_ARG
    assert call([0], pbuf=None) == RV_E_ARG
    assert call([0], dig=None) == RV_E_ARG
    assert L.rv_verify_shard_groups(c.ctx.handle, c.handle, buf, C.c_size_t(len(proof)), None, C.c_uint32(1), _p(out), C.byref(zc)) == RV_E_ARG
