#!/usr/bin/env python3
"""Per-rank time of the sharded verifier on ONE GPU: what each of W GPUs would spend on its groups of the verifier's 32 groups
of eight slots (rv_verify_shard_groups) for the config-4 proof (10^7 gates, 50 MB), for W = 1, 2, 4, 8 and two ways to deal the
groups -- rv_verify_partition (online groups round-robin) and the contiguous split [r*32/W, (r+1)*32/W) -- with the proof bytes
each rank uploads (rv_hook_verify_proof_bytes).  The largest rank's time is the scaling ceiling of rv_verify_sharded before the
all-gather.  Next to it: rv_verify on the same proof and context, and rv_verify_multi with 2 and 8 ranks that share this GPU
through the rccl test shim (tests/rccl_shim) -- its overhead over the sum of its shards, not a scaling figure.
Median of 5 after a warm-up, host clock around calls that end in a synchronisation.  Prints JSON lines."""
import ctypes as C
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402

import circuits  # noqa: E402
import reverie_amd  # noqa: E402
from reverie_amd import _lib  # noqa: E402
from reverie_amd.dist import HipShardBackend, verify_partition  # noqa: E402

REPEAT = 5


def median_ms(fn):
    fn()  # warm-up
    ts = []
    for _ in range(REPEAT):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return statistics.median(ts) * 1e3


def shim():
    path = os.path.join(ROOT, "tests", "rccl_shim", "_build", "librccl_shim.so")
    if not os.path.exists(path):
        os.makedirs(os.path.dirname(path), exist_ok=True)
        subprocess.check_call(["/opt/rocm/bin/hipcc", "-shared", "-fPIC", "-O2", "-std=c++17",
                               os.path.join(ROOT, "tests", "rccl_shim", "rccl_shim.cpp"), "-o", path])
    return path


def main():
    L = _lib.lib()
    prog, wit, wc, _ = circuits.layered_gf2()
    seeds = np.random.default_rng(0x5EED).integers(0, 256, (256, 16), dtype=np.uint8)
    ctx = reverie_amd.Context(0)
    c = reverie_amd.Circuit(prog, wc, ctx)
    proof = bytes(reverie_amd.Proof.new(c, wit, [], seeds=seeds))  # (pageable host memory, as a received proof)
    buf = (C.c_uint8 * len(proof)).from_buffer_copy(proof)
    be = HipShardBackend(c)

    def verify():
        ok = C.c_int()
        _lib.check(L.rv_verify_ex(ctx.handle, c.handle, buf, C.c_size_t(len(proof)), C.c_uint32(0), C.byref(ok)))
        assert ok.value == 1

    before = L.rv_hook_verify_proof_bytes()
    verify()
    uploaded = L.rv_hook_verify_proof_bytes() - before
    print(json.dumps({"rv_verify_ms": round(median_ms(verify), 3), "proof_bytes": len(proof), "uploaded_bytes": uploaded}), flush=True)
    shard_sum = {}
    for world in (1, 2, 4, 8):
        n = 32 // world
        for kind in ("partition", "contiguous"):
            ranks = [verify_partition(world, r) if kind == "partition" else list(range(r * n, (r + 1) * n)) for r in range(world)]
            ms, up = [], []
            for groups in ranks:
                before = L.rv_hook_verify_proof_bytes()
                be.verify_groups(proof, groups)
                up.append(L.rv_hook_verify_proof_bytes() - before)
                ms.append(round(median_ms(lambda: be.verify_groups(proof, groups)), 3))
            if kind == "partition":
                shard_sum[world] = sum(ms)
            print(json.dumps({"world": world, "split": kind, "ms_per_rank": ms, "max_ms": max(ms), "uploaded_bytes_per_rank": up,
                              "groups_per_rank": ranks}), flush=True)
    c.close()
    # rv_verify_multi: W ranks = W host threads on this one GPU (the shim's all-gather is a device copy)
    os.environ["RV_RCCL_PATH"] = shim()  # (read when the library first binds RCCL: no communicator exists before this point)
    for world in (2, 8):
        ctxs = [reverie_amd.Context(0) for _ in range(world)]
        circs = [reverie_amd.Circuit(prog, wc, cx) for cx in ctxs]
        cm = (C.c_void_p * world)()
        _lib.check(L.rv_comm_create_all((C.c_void_p * world)(*[cx.handle for cx in ctxs]), C.c_int(world), cm))
        hcirc = (C.c_void_p * world)(*[x.handle for x in circs])

        def multi():
            ok = C.c_int()
            _lib.check(L.rv_verify_multi(cm, hcirc, C.c_int(world), buf, C.c_size_t(len(proof)), C.c_uint32(0), C.byref(ok)))
            assert ok.value == 1

        t = median_ms(multi)
        print(json.dumps({"rv_verify_multi_ranks": world, "ms": round(t, 3), "sum_of_partition_shards_ms": round(shard_sum[world], 3),
                          "overhead_ms": round(t - shard_sum[world], 3)}), flush=True)
        for i in range(world):
            L.rv_comm_destroy(C.c_void_p(cm[i]))
        for x in circs:
            x.close()
        for cx in ctxs:
            cx.close()


if __name__ == "__main__":
    main()
