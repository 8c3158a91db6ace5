"""Which order of work the single-proof verifier chose (rv_hook_verify_schedule), shape by shape: the answer is the same on
every path, so only the counters tell that a shape still takes the path it is here for.

Counters (cumulative): calls, blob, side-stream proof copy, split64, fused Z64 verifier, overlap, MODE_VERIFY_C, calls whose
proof lay in device memory.  The expected deltas restate the verifier's conditions (csrc/verify.inc, verify_schedule):

    blob       no Z64 gates and the packed host arrays + records fit the 1 MiB input staging buffer; host bytes only
    side copy  not blob and 4 MiB or more of online records to copy; host bytes only
    split64    side copy, fused Z64 verifier, no GF(2) gates, every opened repetition in the first 64 slots, rows of 32 or more
               quad words in multiples of 16
    fused Z64  the circuit is eligible (its device bytes show it), rows of a multiple of 8 quad words, RV_Z64_FUSED_VERIFY not 0
    overlap    not blob, rows of a multiple of 16 quad words, 8192 or more GF(2) mask blocks
    VERIFY_C   what rv_hook_verify_vc_count counts: asserted equal to it at every call, and stated for WIDE

Every shape: the good proof (True, strict and reference-compatible) and one altered proof (a `corr` byte of record 3 flipped:
False), through rv_verify_ex and rv_verify_device, the deltas asserted around every call.  Each shape asserts the thresholds it
is meant to cross, so one that misses them fails instead of testing another path."""
import ctypes as C

import numpy as np
import pytest

import circuits
import proof_mutate
import verify_length_cases as cases
from test_gpu_verify_device import golden, upload
from test_gpu_verify_groups import span_bytes
from test_gpu_verify_lengths import fused_eligible, rv, set_env  # noqa: F401 (rv: fixture)

pytestmark = pytest.mark.gpu

SWITCHES = ("RV_VERIFY_HEAD", "RV_OVERLAP_MIN", "RV_OVERLAP", "RV_Z64_FUSED_VERIFY", "RV_VERIFY_VC", "RV_Z64_FUSED", "RV_AES_COL4")
IN_STAGE_BYTES = 1 << 20  # (rv_ctx::IN_STAGE_BYTES)
SIDE_COPY_BYTES = 4 << 20
OVERLAP_BLOCKS = 8192
# the host arrays of a whole proof in the blob, each segment rounded up to 16 bytes: seeds, omit, keep, onm, the ten opened quad
# words, hkeys, hco, hco64, src
BLOB_ARRAYS = 256 * 16 + 256 + 64 * 4 + 64 * 4 + 48 + 256 * 128 + 256 * 32 + 256 * 32 + 6 * 256 * 8


@pytest.fixture(autouse=True)
def no_switches(monkeypatch):
    for name in SWITCHES:
        monkeypatch.delenv(name, raising=False)


def counters():
    from reverie_amd import _lib

    out = (C.c_uint64 * 8)()
    assert _lib.lib().rv_hook_verify_schedule(out) == 0
    return tuple(int(x) for x in out), int(_lib.lib().rv_hook_verify_vc_count())


def want(blob=0, side=0, split=0, z64f=0, overlap=0, vc=0, dev=0):
    """the deltas of one call (vc None: whatever rv_hook_verify_vc_count says)"""
    return (1, int(blob), int(side), int(split), int(z64f), int(overlap), None if vc is None else int(vc), int(dev))


def counted(call, expect, what):
    """call()'s result, with the schedule counters' deltas asserted"""
    s0, vc0 = counters()
    result = call()
    s1, vc1 = counters()
    delta = tuple(a - b for a, b in zip(s1, s0))
    print(f"[{what}] {delta}")
    assert delta[6] == vc1 - vc0, what
    if expect[6] is None:
        expect = expect[:6] + (delta[6],) + expect[7:]
    assert delta == expect, (what, delta, expect)
    return result


def flip_corr(proof: bytes, domain: int) -> bytes:
    comm, doms = proof_mutate.parse(proof)
    doms = proof_mutate._copy(doms)
    corr = bytearray(doms[domain][0][3][2][1])
    assert len(corr) > 0
    corr[0] ^= 0xFF
    doms[domain][0][3][2][1] = bytes(corr)
    return proof_mutate.serialise(comm, doms)


def check_shape(rv, c, good: bytes, domain: int, host, device, what):
    """both forms on the good and the altered proof"""
    bad = flip_corr(good, domain)
    assert len(bad) == len(good)
    for form, expect, wrap in (("host", host, rv.Proof), ("device", device, lambda data: rv.DeviceProof(upload(data)))):
        pg, pb = wrap(good), wrap(bad)
        for strict in (True, False):
            assert counted(lambda: pg.verify(c, strict=strict), expect, f"{what} {form} good strict={strict}") is True
        assert counted(lambda: pb.verify(c, strict=True), expect, f"{what} {form} altered") is False


def blob_bytes(proof: bytes) -> int:
    """upper bound of what the blob holds: the arrays, the records of the five online groups (one run per domain, each kept at its
    offset modulo 16)"""
    return BLOB_ARRAYS + span_bytes(proof, range(5)) + 4 * 16


def test_small_gf2_blob(rv):
    prog, w2, w64, wc, proof = golden("adder64")
    assert not (prog["domain"] == 1).any() and blob_bytes(proof) <= IN_STAGE_BYTES // 2
    c = rv.Circuit(prog, wc)
    try:
        assert (c.info["gf2_masks"] + 127) // 128 < OVERLAP_BLOCKS
        check_shape(rv, c, proof, 0, want(blob=1, vc=None), want(vc=None, dev=1), "adder64")
    finally:
        c.close()


def test_small_mixed_main_stream(rv, monkeypatch):
    prog, w2, w64, wc, proof = golden("z64_mix")
    assert (prog["domain"] == 1).any() and span_bytes(proof, range(5)) < SIDE_COPY_BYTES // 2
    fused = fused_eligible(rv, prog, wc, monkeypatch)
    c = rv.Circuit(prog, wc)
    try:
        assert (c.info["gf2_masks"] + 127) // 128 < OVERLAP_BLOCKS
        check_shape(rv, c, proof, 1, want(z64f=fused), want(z64f=fused, dev=1), "z64_mix")
    finally:
        c.close()


@pytest.mark.parametrize("vc", (None, "0"))
def test_wide_compact_corrections(rv, rule_seeds, monkeypatch, vc):
    prog, w2, w64, wc = cases.circuit("WIDE")
    c = rv.Circuit(prog, wc)
    try:
        proof = bytes(rv.Proof.new(c, w2, w64, seeds=rule_seeds))
        assert blob_bytes(proof) <= IN_STAGE_BYTES // 2 and (c.info["gf2_masks"] + 127) // 128 < OVERLAP_BLOCKS
        set_env(monkeypatch, {"RV_VERIFY_VC": vc})
        on = vc is None
        check_shape(rv, c, proof, 0, want(blob=1, vc=on), want(vc=on, dev=1), f"WIDE RV_VERIFY_VC={vc}")
    finally:
        c.close()


@pytest.mark.parametrize("fused", (None, "0"))
def test_z64_fused(rv, rule_seeds, monkeypatch, fused):
    prog, w2, w64, wc = cases.circuit("Z")
    assert fused_eligible(rv, prog, wc, monkeypatch)
    c = rv.Circuit(prog, wc)
    try:
        proof = bytes(rv.Proof.new(c, w2, w64, seeds=rule_seeds))
        assert span_bytes(proof, range(5)) < SIDE_COPY_BYTES // 2
        set_env(monkeypatch, {"RV_Z64_FUSED_VERIFY": fused})
        on = fused is None
        check_shape(rv, c, proof, 1, want(z64f=on), want(z64f=on, dev=1), f"Z RV_Z64_FUSED_VERIFY={fused}")
    finally:
        c.close()


# group lists of the 4.8 MB proof for rv_verify_shard_groups, neither contiguous
FEW_GROUPS = [0, 2, 4, 9, 30]  # three online groups: under 4 MiB of records, rows of 10 quad words
HALF_GROUPS = [0, 1, 2, 3, 4, 6, 8, 10, 12, 14, 16, 18, 20, 22, 24, 31]  # every online group: rows of 32 quad words


@pytest.mark.parametrize("fused", (None, "0"))
def test_large_z64_side_copy_and_split(rv, rule_seeds, monkeypatch, fused):
    from reverie_amd.dist import HipShardBackend

    prog, w64, wc = cases.split_circuit()
    assert not (prog["domain"] != 1).any() and fused_eligible(rv, prog, wc, monkeypatch)
    c = rv.Circuit(prog, wc)
    try:
        proof = bytes(rv.Proof.new(c, [], w64, seeds=rule_seeds))
        assert span_bytes(proof, range(5)) >= SIDE_COPY_BYTES and c.info["gf2_masks"] == 0
        set_env(monkeypatch, {"RV_Z64_FUSED_VERIFY": fused})
        on = fused is None
        check_shape(rv, c, proof, 1, want(side=1, split=on, z64f=on), want(z64f=on, dev=1), f"SPLIT RV_Z64_FUSED_VERIFY={fused}")
        # groups: the digests are the whole proof's, whatever the schedule
        be = HipShardBackend(c)
        every, zc = counted(lambda: be.verify_groups(proof, list(range(32))), want(side=1, split=on, z64f=on), "SPLIT all groups")
        assert zc
        assert span_bytes(proof, FEW_GROUPS) < SIDE_COPY_BYTES <= span_bytes(proof, HALF_GROUPS)
        for groups, expect in ((FEW_GROUPS, want()), (HALF_GROUPS, want(side=1, split=on, z64f=on))):
            dig, zc = counted(lambda: be.verify_groups(proof, groups), expect, f"SPLIT groups {groups}")
            assert zc and np.array_equal(dig.reshape(-1, 8, 32), every.reshape(32, 8, 32)[groups])
    finally:
        c.close()


def test_large_gf2_side_unpack_and_overlap(rv, rule_seeds):
    """layered_gf2 of AND gates only, 4096 inputs, 65536 gates per layer: a mask per input and two per AND gate, so 8 layers are
    the fewest with 8192 mask blocks of 128 (7 give 7200); the online records, two bits per AND gate in each, pass 4 MiB at 7"""
    n_in, width = 4096, 65536
    layers = next(n for n in range(1, 64) if (n_in + 2 * width * n + 127) // 128 >= OVERLAP_BLOCKS)
    assert layers == 8
    prog, wit, wc, _ = circuits.layered_gf2(n_in=n_in, width=width, layers=layers, p_and=1.0, fold_to=128)
    c = rv.Circuit(prog, wc)
    try:
        assert c.info["gf2_masks"] == n_in + 2 * width * layers and (c.info["gf2_masks"] + 127) // 128 >= OVERLAP_BLOCKS
        proof = bytes(rv.Proof.new(c, wit, [], seeds=rule_seeds))
        assert span_bytes(proof, range(5)) >= SIDE_COPY_BYTES
        check_shape(rv, c, proof, 0, want(side=1, overlap=1, vc=None), want(overlap=1, vc=None, dev=1), "layered")
    finally:
        c.close()
