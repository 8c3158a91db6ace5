"""What the single-proof prover decided (rv_hook_prove_schedule), shape by shape and entry point by entry point: the proof is
the same on every path, so only the counters tell that a shape still takes the path it is here for.

Counters (cumulative): commitments queued, early, early Z64, direct openings, small staging, stage_in, MODE_PROVE_V, fused Z64,
overlap, lane-distributed mask generator; then per openings call: one launch, heads and inputs in one launch, separate launches,
error word sent by that launch.  The expected deltas restate the prover's conditions (csrc/prove.inc: prove_schedule, ProveRun;
csrc/open.inc: shard_open_impl) for a whole proof, 256 repetitions in rows of 64 quad words:

    early       rv_prove / rv_prove_wdev / rv_prove_batch of one / an rv_prove_ops hit (1024 ops or more, seen before on the context
                with the same knobs); RV_EARLY not 0; the circuit has an early plan (pure GF(2) with RV_EARLY_MIN Mul gates or
                more, or pure Z64 with as many -- its early_staging_bytes are not 0)
    early Z64   early, Z64 plan
    direct      early GF(2); RV_OPEN_DIRECT num/den of the broadcast vector's tiles is not none; tiles of 64 bytes (16 with the knob)
    small       not early, host proof: the framed proof + 64 bytes fit the 1 MiB mapped staging buffer
    stage_in    the commitment's caller waits for the stream itself (every prover; not rv_shard_commit) and 256 seeds + the GF(2)
                witness fit 1 MiB
    PROVE_V     the circuit's vclr_ok (rv_hook_circuit_levels)
    fused Z64   the circuit is eligible (its device bytes show it) and RV_Z64_FUSED is not 0
    overlap     RV_OVERLAP not 0 and RV_OVERLAP_MIN (8192) cipher blocks of 128 masks or more
    col4        GF(2) masks, and overlap or at most 4096 blocks (RV_AES_COL4 unset)
    one launch  pure GF(2), no direct openings, and the three vectors' tiles (open.hip: ex_tb_for) number 2048 at most -- the
                corrections' tiles only where some repetition's corrections are extracted (fewer than 256 staged, or not early)
    heads + in  pure GF(2) otherwise (the input vector's tiles alone number 2048 at most)
    separate    any Z64 vector
    error word  one launch, small staging

Every shape asserts the thresholds it is meant to cross, so one that misses them fails instead of testing another path.  Proof
bytes are the oracle's (computed once per shape)."""
import ctypes as C

import numpy as np
import pytest

import circuits
import proof_mutate
from test_gpu_verify_lengths import fused_eligible, set_env

pytestmark = pytest.mark.gpu

SWITCHES = ("RV_EARLY", "RV_EARLY_MIN", "RV_EARLY_REPS", "RV_EARLY_CHUNKS", "RV_OPEN_DIRECT", "RV_OVERLAP", "RV_OVERLAP_MIN", "RV_Z64_FUSED",
            "RV_AES_COL4", "RV_VCLR", "RV_OPS_CACHE", "RV_EARLY_POISON")
STAGE_BYTES = 1 << 20  # (rv_ctx::STAGE_BYTES, rv_ctx::IN_STAGE_BYTES)
OVERLAP_BLOCKS, COL4_SMALL_BLOCKS = 8192, 4096
OPS_CACHE_MIN_OPS = 1024
NAMES = ("calls", "early", "early_z64", "direct", "small", "stage_in", "vclr", "z64f", "overlap", "col4", "one", "heads_in", "separate", "err_word")


@pytest.fixture(scope="module")
def rv():
    import reverie_amd

    reverie_amd.Context.default()
    return reverie_amd


@pytest.fixture(scope="module")
def ctx(rv):
    """a context of the test's own: its staging buffers, mailbox and ops cache start empty"""
    cx = rv.Context(0)
    yield cx
    cx.close()


@pytest.fixture(autouse=True)
def no_switches(monkeypatch):
    for name in SWITCHES:
        monkeypatch.delenv(name, raising=False)


def lib():
    from reverie_amd import _lib

    return _lib.lib()


def counters():
    out = (C.c_uint64 * 16)()
    assert lib().rv_hook_prove_schedule(out) == 0
    assert out[14] == 0 and out[15] == 0
    return tuple(int(x) for x in out[:14])


def counted(call, expect, what):
    """call()'s result (an exception it raised is returned), with the schedule counters' deltas asserted"""
    before = counters()
    try:
        result = call()
    except Exception as e:  # noqa: BLE001 (the caller looks at it)
        result = e
    delta = dict(zip(NAMES, (a - b for a, b in zip(counters(), before))))
    print(f"[{what}] {delta}")
    assert delta == expect, (what, delta, expect)
    return result


def tiles(n_bytes, cap=128):
    """open.hip, ex_tb_for: workgroups of a vector of n_bytes"""
    tb = cap
    while tb > 8 and (n_bytes + tb - 1) // tb < 2048:
        tb //= 2
    return (n_bytes + tb - 1) // tb, tb


def vector_bytes(proof):
    """(rec, corr, in) lengths of the first online record of each domain"""
    _, ((recs2, _), (recs64, _)) = proof_mutate.parse(proof)
    return tuple(len(v) for v in recs2[0][2]), tuple(len(v) for v in recs64[0][2])


def opening(proof, corrections=True, direct=False, err_word=False):
    """the openings' form for this proof"""
    (r, c, i), z = vector_bytes(proof)
    form = dict(one=0, heads_in=0, separate=0, err_word=0)
    if any(z):
        form["separate"] = 1
    elif not direct and tiles(r, 256)[0] + (tiles(c)[0] if corrections else 0) + tiles(i, 256)[0] <= 2048:
        form["one"] = 1
        form["err_word"] = int(err_word)
    else:
        assert tiles(i, 256)[0] <= 2048
        form["heads_in"] = 1
    return form


def vclr_ok(c):
    n, ok = C.c_size_t(), C.c_int()
    assert lib().rv_hook_circuit_levels(c.handle, None, C.c_size_t(0), C.byref(n), C.byref(ok), None) == 0
    return bool(ok.value)


class Shape:
    """a circuit on the test's context with the oracle's proof, and what a commitment of it decides as the environment stands"""

    def __init__(self, rv, ctx, oracle, seeds, monkeypatch, prog, w2, w64, wc, env=None):
        self.rv, self.ctx, self.seeds, self.prog, self.wc = rv, ctx, seeds, prog, wc
        self.w2, self.w64 = np.asarray(w2, np.uint8), np.asarray([int(x) for x in w64], np.uint64)
        self.has64 = bool((prog["domain"] == 1).any())
        self.fused_ok = self.has64 and fused_eligible(rv, prog, wc, monkeypatch)
        self.env = dict(env or {})
        set_env(monkeypatch, self.env)
        self.want = oracle.prove(prog, list(self.w2), [int(x) for x in self.w64], wc, seeds, threads=4)
        self.c = rv.Circuit(prog, wc, ctx=ctx)
        self.c_ops = rv.Circuit(prog, wc, ctx=ctx, whole_prover=True)  # (what rv_prove_ops compiles)

    def close(self):
        self.c.close()
        self.c_ops.close()

    def commit(self, c=None, stage_in=True):
        info = (c or self.c).info
        blocks = (info["gf2_masks"] + 127) // 128
        overlap = self.env.get("RV_OVERLAP") != "0" and blocks >= int(self.env.get("RV_OVERLAP_MIN", OVERLAP_BLOCKS))
        return dict(calls=1, stage_in=int(stage_in and 256 * 16 + info["gf2_inputs"] <= STAGE_BYTES), vclr=int(vclr_ok(c or self.c)),
                    z64f=int(self.fused_ok and self.env.get("RV_Z64_FUSED") != "0"), overlap=int(overlap),
                    col4=int(blocks > 0 and (overlap or blocks <= COL4_SMALL_BLOCKS)))

    def plan(self, c=None):
        """(early plan taken, staged repetitions) as the environment stands"""
        if self.env.get("RV_EARLY") == "0" or not (c or self.c).info["early_staging_bytes"]:
            return False, 0
        return True, int(self.env.get("RV_EARLY_REPS", 128 if self.has64 else 256))

    def direct(self):
        """whether an early GF(2) proof's broadcast vectors go straight to the proof buffer"""
        knob = self.env.get("RV_OPEN_DIRECT")
        num, den = (int(x) for x in knob.split("/")) if knob else (1, 1)
        n_tiles, tb = tiles(vector_bytes(self.want)[0][0], 256)
        return not self.has64 and n_tiles * num // den > 0 and tb >= (16 if knob else 64)

    def host(self, allow_early=True, c=None):
        """rv_prove and the entry points that end in it"""
        e = dict.fromkeys(NAMES, 0)
        e.update(self.commit(c))
        early, reps = self.plan(c)
        if early and allow_early:
            e["early"], e["early_z64"] = 1, int(self.has64)
            e["direct"] = int(self.direct())
            e.update(opening(self.want, corrections=self.has64 or reps < 256, direct=bool(e["direct"])))
        else:
            e["small"] = int(len(self.want) + 64 <= STAGE_BYTES)
            e.update(opening(self.want, err_word=bool(e["small"])))
        return e

    def device(self):
        """rv_prove_device, rv_prove_batch_device of one: the openings stay in device memory"""
        e = dict.fromkeys(NAMES, 0)
        e.update(self.commit())
        e.update(opening(self.want))
        return e

    def gpu_witness(self, w2, w64, batched=False):
        import torch

        g = torch.from_numpy(np.asarray(w2, np.uint8).copy()).cuda() if len(w2) else None
        z = torch.from_numpy(np.asarray(w64, np.uint64).view(np.int64).copy()).cuda() if len(w64) else None
        return (g[None] if batched and g is not None else g), (z[None] if batched and z is not None else z)

    def entry_points(self, w2, w64, wdev=True):
        """(name, call -> proof bytes, expected deltas) of every entry point that reaches the single-proof prover"""
        rv, c, s = self.rv, self.c, self.seeds
        eps = [("rv_prove", lambda: bytes(rv.Proof.new(c, w2, w64, seeds=s)), self.host()),
               ("rv_prove_device", lambda: bytes(rv.DeviceProof.new(c, w2, w64, seeds=s).to_proof()), self.device()),
               ("rv_prove_batch[1]", lambda: bytes(rv.Proof.new_batch(c, w2[None], w64[None], seeds=s[None])[0]), self.host()),
               ("rv_prove_batch_device[1]", lambda: rv.prove_batch_device(c, w2[None], w64[None], seeds=s[None])[0].tensor.cpu().numpy().tobytes(),
                self.device())]
        if wdev and (len(w2) or len(w64)):
            g, z = self.gpu_witness(w2, w64)
            eps += [("rv_prove_wdev", lambda: bytes(rv.Proof.new(c, g, z, seeds=s)), self.host()),
                    ("rv_prove_device_wdev", lambda: bytes(rv.DeviceProof.new(c, g, z, seeds=s).to_proof()), self.device())]
        return eps

    def bad_witness(self):
        """a witness the cleartext evaluator refuses, one input changed"""
        for k in range(min(64, len(self.w2) + len(self.w64))):
            w2, w64 = self.w2.copy(), self.w64.copy()
            if k < len(w2):
                w2[k] ^= 1
            else:
                w64[k - len(w2)] ^= np.uint64(1)
            if not self.c.evaluate(w2, w64).ok:
                return w2, w64
        raise AssertionError("no single changed input makes the statement false")

    def check(self, invalid=True):
        """every entry point: the oracle's bytes, then (invalid) code 1 for a false statement and a good proof again"""
        bad = self.bad_witness() if invalid else None
        for name, call, expect in self.entry_points(self.w2, self.w64):
            assert counted(call, expect, name) == self.want, name
        for (name, call, expect), (_, again, _) in zip(self.entry_points(*bad, wdev=False) if bad else (), self.entry_points(self.w2, self.w64, wdev=False)):
            err = counted(call, expect, name + " invalid witness")
            assert isinstance(err, self.rv.ReverieError) and err.code == 1, (name, err)
            assert counted(again, expect, name + " after it") == self.want, name
        # rv_prove_ops: the first call compiles (no early corrections), the second finds the circuit
        hit = len(self.prog) >= OPS_CACHE_MIN_OPS
        ops = lambda: bytes(self.rv.Proof.new(self.prog, self.w2, self.w64, self.wc, seeds=self.seeds, ctx=self.ctx))  # noqa: E731
        assert lib().rv_ctx_ops_cache_clear(self.ctx.handle) == 0  # (the context may know the program from another case)
        hits = lib().rv_hook_ops_cache_hits()
        assert counted(ops, self.host(allow_early=False, c=self.c_ops), "rv_prove_ops miss") == self.want
        assert counted(ops, self.host(allow_early=hit, c=self.c_ops), "rv_prove_ops again") == self.want
        assert lib().rv_hook_ops_cache_hits() == hits + int(hit)


def test_tiny_gf2_small_staging_one_launch(rv, ctx, oracle, rule_seeds, monkeypatch):
    prog, wit, wc, st = circuits.layered_gf2(n_in=40, width=96, layers=5, p_and=0.6, fold_to=6)
    assert 100 <= st["and"] <= 500
    s = Shape(rv, ctx, oracle, rule_seeds, monkeypatch, prog, wit, [], wc)
    try:
        assert len(s.want) + 64 <= STAGE_BYTES and not s.plan()[0]
        assert s.host() == dict(s.host(), small=1, stage_in=1, one=1, err_word=1, col4=1, overlap=0, early=0)
        assert s.device() == dict(s.device(), one=1, err_word=0, small=0)
        s.check()
        # the same circuit through rv_shard_commit: the commitment waits for the device itself, nothing is staged, nothing opened
        from reverie_amd.dist import HipShardBackend

        be = HipShardBackend(s.c)
        expect = dict(dict.fromkeys(NAMES, 0), **s.commit(stage_in=False))
        assert expect["stage_in"] == 0
        shard = counted(lambda: be.commit(list(s.w2), [], rule_seeds, 0, 256), expect, "rv_shard_commit")
        assert not isinstance(shard, Exception), shard
        be.destroy(shard)
    finally:
        s.close()


@pytest.mark.parametrize("env,early,overlap", [({"RV_EARLY": "0"}, 0, 0), ({"RV_EARLY": "2", "RV_EARLY_MIN": "1000"}, 1, 0),
                                               ({"RV_EARLY": "0", "RV_OVERLAP_MIN": "1000"}, 0, 1),
                                               ({"RV_EARLY": "0", "RV_OVERLAP_MIN": "1000", "RV_OVERLAP": "0"}, 0, 0)])
def test_large_gf2_plain_early_overlap(rv, ctx, oracle, rule_seeds, monkeypatch, env, early, overlap):
    prog, wit, wc, st = circuits.layered_gf2(n_in=64, width=8192, layers=40, p_and=0.5, fold_to=16)
    s = Shape(rv, ctx, oracle, rule_seeds, monkeypatch, prog, wit, [], wc, env)
    try:
        blocks = (s.c.info["gf2_masks"] + 127) // 128
        assert len(s.want) > STAGE_BYTES and st["and"] >= 1000 and 1000 <= blocks <= COL4_SMALL_BLOCKS
        # plain: the device-to-host copy, heads and inputs in one launch; early with all 256 repetitions staged: no corrections to extract
        assert s.host() == dict(s.host(), early=early, small=0, err_word=0, overlap=overlap, col4=1, one=0, heads_in=1, direct=0)
        s.check(invalid=bool(early) or "RV_OVERLAP_MIN" not in env)
    finally:
        s.close()


def test_early_staged_and_unstaged_repetitions(rv, ctx, oracle, rule_seeds, monkeypatch):
    prog, wit, wc, st = circuits.layered_gf2(n_in=37, width=4736, layers=70, p_and=0.6, fold_to=37)
    s = Shape(rv, ctx, oracle, rule_seeds, monkeypatch, prog, wit, [], wc, {"RV_EARLY": "2", "RV_EARLY_MIN": "1000", "RV_EARLY_REPS": "96"})
    try:
        assert s.plan() == (True, 96) and len(s.want) > STAGE_BYTES
        assert s.host() == dict(s.host(), early=1, early_z64=0, heads_in=1)
        s.check(invalid=False)
    finally:
        s.close()


@pytest.mark.parametrize("knob,direct", [("1/1", 1), ("0/1", 0)])
def test_early_direct_openings(rv, ctx, oracle, rule_seeds, monkeypatch, knob, direct):
    prog, wit, wc, st = circuits.layered_gf2(n_in=64, width=16384, layers=36, p_and=0.5, fold_to=16)
    s = Shape(rv, ctx, oracle, rule_seeds, monkeypatch, prog, wit, [], wc, {"RV_EARLY": "2", "RV_EARLY_MIN": "1000", "RV_OPEN_DIRECT": knob})
    try:
        blocks = (s.c.info["gf2_masks"] + 127) // 128
        n_tiles, tb = tiles(vector_bytes(s.want)[0][0], 256)
        assert s.plan()[0] and tb >= 16 and n_tiles > 1 and COL4_SMALL_BLOCKS < blocks < OVERLAP_BLOCKS
        assert s.host() == dict(s.host(), early=1, direct=direct, heads_in=1, col4=0, overlap=0)
        s.check(invalid=False)
    finally:
        s.close()


@pytest.mark.parametrize("fused", (None, "0"))
def test_small_z64_separate_launches(rv, ctx, oracle, rule_seeds, monkeypatch, fused):
    prog, w64, wc, st = circuits.layered_z64(n_in=16, width=64, n_mul=300)
    s = Shape(rv, ctx, oracle, rule_seeds, monkeypatch, prog, [], w64, wc, {"RV_Z64_FUSED": fused} if fused else {})
    try:
        assert s.fused_ok and len(s.want) + 64 <= STAGE_BYTES and not s.plan()[0]
        assert s.host() == dict(s.host(), small=1, separate=1, err_word=0, z64f=int(fused is None), col4=0, vclr=0)
        s.check()
    finally:
        s.close()


@pytest.mark.parametrize("fused", (None, "0"))
def test_early_z64(rv, ctx, oracle, rule_seeds, monkeypatch, fused):
    prog, w64, wc, st = circuits.layered_z64(n_in=64, width=2048, n_mul=24000)
    env = {"RV_EARLY": "2", "RV_EARLY_MIN": "1000", "RV_EARLY_REPS": "64", "RV_EARLY_CHUNKS": "5"}
    s = Shape(rv, ctx, oracle, rule_seeds, monkeypatch, prog, [], w64, wc, dict(env, RV_Z64_FUSED=fused) if fused else env)
    try:
        assert st["mul"] % 2 == 0 and s.plan() == (True, 64) and s.fused_ok and len(s.want) > STAGE_BYTES
        assert s.host() == dict(s.host(), early=1, early_z64=1, direct=0, separate=1, z64f=int(fused is None))
        s.check(invalid=fused is None)
    finally:
        s.close()


def test_small_mixed_circuit(rv, ctx, oracle, rule_seeds, monkeypatch):
    prog, w2, w64, wc = circuits.random_mixed(np.random.default_rng(3))
    assert (prog["domain"] == 1).any() and (prog["domain"] == 0).any()
    s = Shape(rv, ctx, oracle, rule_seeds, monkeypatch, prog, w2, w64, wc)
    try:
        assert not s.plan()[0] and len(s.want) + 64 <= STAGE_BYTES
        assert s.host() == dict(s.host(), small=1, separate=1, err_word=0, early=0, vclr=0)
        s.check(invalid=False)  # (its assertions sit on values the generator knows; a changed input need not break one)
    finally:
        s.close()
