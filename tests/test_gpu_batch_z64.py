"""rv_prove_batch / rv_verify_batch on Z64 and mixed circuits: the one-pass path (batched Z64 level launches, recorded Z64
phase kernels) must give exactly what rv_prove / rv_verify_ex give proof by proof, and the CPU oracle."""
import ctypes as C

import numpy as np
import pytest

import circuits
import z64_batch_circuits as zc
from reverie_amd.ops import Z64, program

pytestmark = pytest.mark.gpu

PH_INTERP = 2


@pytest.fixture(scope="module")
def rv():
    import reverie_amd

    reverie_amd.Context.default()  # raises loudly if the HIP library or the GPU is missing
    return reverie_amd


def _seeds(rng, n):
    return rng.integers(0, 256, (n, 256, 16), dtype=np.uint8)


def _interp_launches(rv, fn):
    """RV_PH_INTERP launches counted while fn() runs"""
    from reverie_amd import _lib

    L = _lib.lib()
    ctx = rv.Context.default()
    L.rv_ctx_profile(ctx.handle, 1, 1, None)
    try:
        out = fn()
    finally:
        prof = _lib.Profile()
        L.rv_ctx_profile(ctx.handle, 0, 0, C.byref(prof))
    return int(prof.launches[PH_INTERP]), out


def test_batch_z64_launches_per_level(rv):
    """A deep, narrow pure-Z64 circuit: one pass issues each level once for the whole batch, so the interpreter's launch
    count is at most the level count and the same for 4 and 32 proofs (one proof after another would give B x levels)."""
    prog, wit, wc = zc.chain_z64()
    c = rv.Circuit(prog, wc)
    levels = c.info["levels"]
    rng = np.random.default_rng(11)
    counts, vcounts = [], []
    for B in (4, 32):
        seeds = _seeds(rng, B)
        wits = np.tile(np.asarray(wit, np.uint64), (B, 1))
        n, proofs = _interp_launches(rv, lambda: rv.Proof.new_batch(c, np.zeros((B, 0), np.uint8), wits, seeds=seeds))
        assert 1 <= n <= levels, (B, n, levels)
        counts.append(n)
        nv, ok = _interp_launches(rv, lambda: rv.verify_batch(c, proofs))
        assert ok == [True] * B
        assert 1 <= nv <= levels, (B, nv, levels)
        vcounts.append(nv)
        assert bytes(proofs[-1]) == bytes(rv.Proof.new(c, [], wit, seeds=seeds[-1]))
    assert counts[0] == counts[1] and vcounts[0] == vcounts[1]


def _cases():
    prog, wit, wc = zc.chain_z64()
    yield "chain", prog, lambda b: [], lambda b: wit, wc
    prog, wit, wc = zc.random_gates_z64()
    yield "random", prog, lambda b: [], lambda b: wit, wc
    prog, wit, wc = zc.layered_small()
    yield "layered", prog, lambda b: [], lambda b: wit, wc
    for seed in (1, 5, 9):
        prog, w2, w64, wc = zc.mixed(seed)
        yield f"mixed{seed}", prog, (lambda b, w2=w2: w2), (lambda b, w64=w64: w64), wc


@pytest.mark.parametrize("case", ["chain", "random", "layered", "mixed1", "mixed5", "mixed9"])
def test_prove_batch_z64_equals_single_proofs(rv, oracle, case):
    """Every batched proof equals Proof.new for the same witness and seeds (B = 2, 3, 17); the first and the last of each
    batch also equal the oracle's."""
    name, prog, w2, w64, wc = next(x for x in _cases() if x[0] == case)
    c = rv.Circuit(prog, wc)
    rng = np.random.default_rng(sum(map(ord, case)))
    for B in (2, 3, 17):
        seeds = _seeds(rng, B)
        g = np.array([w2(b) for b in range(B)], np.uint8).reshape(B, -1)
        z = np.array([w64(b) for b in range(B)], np.uint64).reshape(B, -1)
        got = rv.Proof.new_batch(c, g, z, seeds=seeds)
        assert len(got) == B
        for b in range(B):
            assert bytes(got[b]) == bytes(rv.Proof.new(c, g[b], z[b], seeds=seeds[b])), (case, B, b)
        for b in (0, B - 1):
            assert bytes(got[b]) == oracle.prove(prog, g[b], z[b], wc, seeds[b], threads=4), (case, B, b)


def test_prove_batch_z64_witness_forms(rv, oracle):
    """Witness rows wider than needed, n_gf2 = 0, a circuit without Z64 inputs; a bad witness fails the whole call with
    no proofs; OS seeds verify; single / batch / single on one context give the same bytes."""
    from reverie_amd._lib import ReverieError

    rng = np.random.default_rng(23)
    prog, wit, wc = zc.chain_z64(lanes=3, rounds=20)
    c = rv.Circuit(prog, wc)
    B = 5
    seeds = _seeds(rng, B)
    wide = np.full((B, len(wit) + 5), 0xDEADBEEF, np.uint64)  # (columns past the inputs are never read)
    wide[:, :len(wit)] = np.asarray(wit, np.uint64)
    got = rv.Proof.new_batch(c, np.ones((B, 3), np.uint8), wide, seeds=seeds)  # (GF(2) rows wider than the circuit's zero inputs)
    for b in range(B):
        assert bytes(got[b]) == bytes(rv.Proof.new(c, [], wit, seeds=seeds[b]))
    assert bytes(got[4]) == oracle.prove(prog, [], wit, wc, seeds[4], threads=4)
    # no Z64 inputs at all
    ops = [Z64.Const(0, 5), Z64.Const(1, 7), Z64.Mul(2, 0, 1), Z64.SubConst(3, 2, 35), Z64.AssertZero(3), Z64.Random(4),
           Z64.Mul(5, 4, 2), Z64.Add(6, 5, 5), Z64.Mul(7, 2, 2), Z64.SubConst(8, 7, 1225), Z64.AssertZero(8)]
    p0 = program(ops)
    c0 = rv.Circuit(p0, (9, 0))
    g0 = rv.Proof.new_batch(c0, np.zeros((3, 0), np.uint8), np.zeros((3, 0), np.uint64), seeds=seeds[:3])
    for b in range(3):
        assert bytes(g0[b]) == oracle.prove(p0, [], [], (9, 0), seeds[b], threads=2)
        assert g0[b].verify(c0, strict=True)
    # one bad witness: code 1, no proofs
    bad = np.tile(np.asarray(wit, np.uint64), (4, 1))
    bad[2, 1] ^= 1
    with pytest.raises(ReverieError) as e:
        rv.Proof.new_batch(c, np.zeros((4, 0), np.uint8), bad, seeds=seeds[:4])
    assert e.value.code == 1
    # OS randomness
    pm, w2, w64, wcm = zc.mixed(3)
    cm = rv.Circuit(pm, wcm)
    anon = rv.Proof.new_batch(cm, np.tile(np.asarray(w2, np.uint8), (6, 1)), np.tile(np.asarray(w64, np.uint64), (6, 1)))
    assert len({bytes(p) for p in anon}) == 6
    assert all(p.verify(cm, strict=True) for p in anon)
    assert rv.verify_batch(cm, anon) == [True] * 6
    # single, batch, single on one context
    one = bytes(rv.Proof.new(cm, w2, w64, seeds=seeds[0]))
    mid = rv.Proof.new_batch(cm, np.tile(np.asarray(w2, np.uint8), (2, 1)), np.tile(np.asarray(w64, np.uint64), (2, 1)), seeds=seeds[:2])
    assert bytes(mid[0]) == one == bytes(rv.Proof.new(cm, w2, w64, seeds=seeds[0]))


def test_prove_batch_z64_chunks(rv, monkeypatch):
    """RV_BATCH_MAX=4 splits a batch of 11 into passes of at most 4: the same bytes as the default (one pass) and as single
    proofs, whatever order the proofs are released in, with a new batch in between."""
    prog, w2, w64, wc = zc.mixed(7, n_gates=400)
    c = rv.Circuit(prog, wc)
    rng = np.random.default_rng(99)
    nb = 11
    seeds = _seeds(rng, nb)
    g = np.tile(np.asarray(w2, np.uint8), (nb, 1))
    z = np.tile(np.asarray(w64, np.uint64), (nb, 1))
    want = [bytes(rv.Proof.new(c, w2, w64, seeds=seeds[b])) for b in range(nb)]
    for env in ({}, {"RV_BATCH_MAX": "4"}, {"RV_BATCH_MAX": "4", "RV_BATCH_COPY_OUT": "1"}):
        for k in ("RV_BATCH_MAX", "RV_BATCH_COPY_OUT"):
            monkeypatch.delenv(k, raising=False)
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        got = rv.Proof.new_batch(c, g, z, seeds=seeds)
        keep = [bytes(p) for p in got]
        del got[::2]
        again = rv.Proof.new_batch(c, g[:3], z[:3], seeds=seeds[:3])
        assert [bytes(p) for p in got] == keep[1::2]
        del got
        assert keep == want and [bytes(p) for p in again] == want[:3]


def _z64_offsets(c, blob):
    """(start of the z64 online section, its record size, start of the z64 preprocessing section) of a proof of c"""
    sz2, sz64 = c.record_sizes()
    on64 = 32 + 8 + 40 * sz2 + 8 + 216 * 48 + 8
    pre64 = on64 + 40 * sz64 + 8
    assert pre64 + 216 * 48 == len(blob)
    return on64, sz64, pre64


def _single(rv, c, blob, strict):
    from reverie_amd._lib import ReverieError

    try:
        return rv.Proof(blob).verify(c, strict=strict)
    except ReverieError as e:
        assert e.code == 4
        return None


@pytest.mark.parametrize("case", ["chain", "mixed5"])
def test_verify_batch_z64_matches_single_verifier(rv, oracle, monkeypatch, case):
    """verify_batch answers, proof by proof, what rv_verify_ex answers (strict and compat) and the oracle: valid proofs, a
    flipped byte in a Z64 online and in a Z64 preprocessing record, a truncated proof, a wrong and an out-of-range omit,
    all in one call; chunked as well."""
    name, prog, w2, w64, wc = next(x for x in _cases() if x[0] == case)
    c = rv.Circuit(prog, wc)
    rng = np.random.default_rng(5)
    nb = 8
    seeds = _seeds(rng, nb)
    g = np.array([w2(b) for b in range(nb)], np.uint8).reshape(nb, -1)
    z = np.array([w64(b) for b in range(nb)], np.uint64).reshape(nb, -1)
    proofs = rv.Proof.new_batch(c, g, z, seeds=seeds)
    assert rv.verify_batch(c, proofs, strict=True) == [True] * nb
    blobs = [bytes(p) for p in proofs]
    on64, sz64, pre64 = _z64_offsets(c, blobs[0])
    b = bytearray(blobs[1]); b[on64 + 4 * sz64 - 1] ^= 0x04; blobs[1] = bytes(b)  # Z64 online record 3 (the last byte of its inputs)
    b = bytearray(blobs[2]); b[on64 + 7 * sz64 + 40] ^= 0x80; blobs[2] = bytes(b)  # Z64 online record 7 (an opened key)
    b = bytearray(blobs[3]); b[pre64 + 48 * 11 + 3] ^= 0x01; blobs[3] = bytes(b)  # Z64 preprocessing record 11 (its seed)
    blobs[4] = blobs[4][:len(blobs[4]) // 2]  # truncated
    b = bytearray(blobs[5]); b[on64 + 2 * sz64] = (b[on64 + 2 * sz64] + 1) % 8; blobs[5] = bytes(b)  # another player omitted
    b = bytearray(blobs[6]); b[on64] = 9; blobs[6] = bytes(b)  # omit out of range
    for env in ({}, {"RV_BATCH_MAX": "3"}):
        monkeypatch.delenv("RV_BATCH_MAX", raising=False)
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        for strict in (False, True):
            want = [_single(rv, c, bl, strict) for bl in blobs]
            assert want[0] is True and want[7] is True and want[4] is None and not want[1] and not want[3]
            assert rv.verify_batch(c, blobs, strict=strict) == [bool(w) for w in want], (strict, want)
            good = [bl for bl, w in zip(blobs, want) if w is not None]
            assert rv.verify_batch(c, good, strict=strict) == [w for w in want if w is not None]
            assert [oracle.verify(prog, wc, bl, strict=strict) for bl, w in zip(blobs, want) if w is not None] == \
                [w for w in want if w is not None]
    monkeypatch.delenv("RV_BATCH_MAX", raising=False)


def test_verify_batch_z64_assertion_gap(rv, oracle):
    """A proof of one statement checked against another that differs only in the constants before its AssertZero gates
    (GF(2) and Z64): accepted in compat mode only, in the batch as alone."""
    c1p, c2p, w2, w64, wc = circuits.assert_circuits()
    c1, c2 = rv.Circuit(c1p, wc), rv.Circuit(c2p, wc)
    seeds = _seeds(np.random.default_rng(8), 4)
    proofs = rv.Proof.new_batch(c1, np.tile(np.asarray(w2, np.uint8), (4, 1)), np.tile(np.asarray(w64, np.uint64), (4, 1)), seeds=seeds)
    assert bytes(proofs[3]) == oracle.prove(c1p, w2, w64, wc, seeds[3], threads=2)
    assert rv.verify_batch(c1, proofs) == [True] * 4
    assert rv.verify_batch(c2, proofs, strict=False) == [p.verify(c2, strict=False) for p in proofs] == [True] * 4
    assert rv.verify_batch(c2, proofs, strict=True) == [p.verify(c2, strict=True) for p in proofs] == [False] * 4
    mixed = [proofs[0], bytes(proofs[1])[:100], proofs[2]]
    assert rv.verify_batch(c2, mixed, strict=False) == [True, False, True]
    assert oracle.verify(c2p, wc, bytes(proofs[0]), strict=False) and not oracle.verify(c2p, wc, bytes(proofs[0]), strict=True)
