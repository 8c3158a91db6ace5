"""The library's multi-rank verifier (rv_verify_sharded / rv_verify_multi, csrc/comm.inc) with MORE THAN ONE rank on one GPU: a
fresh process binds the rccl test shim (tests/rccl_shim: ranks = host threads sharing the GPU, the all-gather as device copies
between them) through RV_RCCL_PATH, as tests/test_gpu_multirank.py does for the prover.  Honest, false, forged, touched and
truncated proofs: every rank must come to rv_verify_ex's (rc, ok).  And LibComm.verify with a real communicator of one rank."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import circuits
from test_gpu_multirank import build_shim

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WORKER = os.path.join(ROOT, "tests", "verify_multirank_worker.py")


def run_worker(args, timeout, **extra):
    env = dict(os.environ, RV_RCCL_PATH=build_shim(), **extra)
    r = subprocess.run([sys.executable, WORKER, *args], env=env, capture_output=True, text=True, timeout=timeout)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    return json.loads(r.stdout.strip().splitlines()[-1])


def test_rv_verify_multi_with_several_ranks_on_one_gpu():
    res = run_worker(["2", "4", "8"], timeout=600)
    assert res and all(res.values()), res
    for n in (2, 4, 8):
        for case in ("mixed", "mixed-flipped", "mixed-truncated", "layered", "false-statement", "forged-omit"):
            assert res["%s/%d/strict" % (case, n)] and res["%s/%d/compat" % (case, n)], (case, n)


def test_rv_verify_multi_full_size_config4():
    """config 4 at full size (10^7 gates): rv_prove's 50 MB proof verified by 2 and 8 ranks sharing the GPU, and again with one
    byte of the last online record's broadcast vector flipped"""
    res = run_worker(["2", "8"], timeout=900, MULTI_FULL="1")
    assert res == {"%s/%d/%s" % (c, n, f): True for c in ("config4", "config4-flipped") for n in (2, 8) for f in ("strict", "compat")}, res


def test_library_communicator_verify_world1(oracle, rule_seeds):
    """LibComm.verify = rv_verify_sharded over a real communicator of one rank (no shim): rv_verify_ex's answers"""
    import reverie_amd as rv
    from reverie_amd.dist import LibComm

    rng = np.random.default_rng(31)
    prog, w2, w64, wc = circuits.random_mixed(rng, n_gates=300)
    c = rv.Circuit(prog, wc)
    proof = rv.Proof.new(c, w2, w64, seeds=rule_seeds)
    lc = LibComm(c)
    assert (lc.rank, lc.world) == (0, 1)
    assert lc.verify(proof) and lc.verify(bytes(proof), strict=False)
    cm1, cm2, a2, a64, wcm = circuits.assert_circuits()
    c2 = rv.Circuit(cm2, wcm)
    false_proof = bytes(rv.Proof.new(cm1, a2, a64, wcm, seeds=rule_seeds))
    lc2 = LibComm(c2)
    assert (lc2.verify(false_proof), lc2.verify(false_proof, strict=False)) == (False, True)
    assert (oracle.verify(cm2, wcm, false_proof, strict=True), oracle.verify(cm2, wcm, false_proof)) == (False, True)
    with pytest.raises(rv.ReverieError) as e:
        lc.verify(bytes(proof)[:100])
    assert e.value.code == 4  # RV_E_PROOF_MALFORMED, as rv_verify_ex
    # another context's circuit is an argument error
    other = rv.Circuit(prog, wc, rv.Context(0))
    from reverie_amd import _lib

    ok = C.c_int()
    buf = (C.c_uint8 * len(proof)).from_buffer_copy(bytes(proof))
    assert _lib.lib().rv_verify_sharded(lc.handle, other.handle, buf, C.c_size_t(len(proof)), C.c_uint32(0), C.byref(ok)) == 9
    lc.close()
    lc2.close()
