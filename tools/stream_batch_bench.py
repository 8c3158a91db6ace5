"""Batches over one stream (rv_prove_streaming_batch) against B single streams (rv_prove_streaming) on configs 4 and 5.

    python tools/stream_batch_bench.py             # both configs, each in a process of its own under a time limit
    python tools/stream_batch_bench.py --step 4    # one config in this process (what the driver runs)

Config 4: the 10^7-gate circuit with recycled wire indices, the default 2^18-op chunks.  Config 5: 10^6 Z64 MUL, 2^16-op chunks.
Every proof of a batch has the same witness (the circuits end in AssertZero gates) and seeds of its own.  For B = 1, 2, 4, 8: wall ms per call (median of three after a warm-up), ms per proof, the device bytes rv_stream_info reports
(wire stores + chunk working sets + incremental trees + proofs + kept transcripts), and every proof byte-compared with the single
stream's; beside them B x one rv_prove_streaming call.  One JSON line per config."""
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402

BATCHES = (1, 2, 4, 8)


def _device_bytes(info):
    return info["wire_store_bytes"] + info["peak_chunk_bytes"] + info["hash_state_bytes"] + info["proof_bytes"] + (info["kept_mib"] << 20)


def _median_ms(fn, reps=3):
    fn()  # (warm-up: sizes the context's staging buffers, starts the worker threads)
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        out = fn()
        ts.append(time.perf_counter() - t0)
    return sorted(ts)[len(ts) // 2] * 1e3, out


def step(config: int) -> dict:
    import circuits
    import reverie_amd
    from reverie_amd.stream import prove_streaming, prove_streaming_batch

    ctx = reverie_amd.Context.default()
    rng = np.random.default_rng(12)
    if config == 4:
        prog, wit, wc, st = circuits.layered_gf2(recycle=True)
        chunk = 1 << 18
        W2 = np.tile(np.asarray(wit, np.uint8), (max(BATCHES), 1))
        W64 = np.zeros((max(BATCHES), 0), np.uint64)
    else:
        prog, w64, wc, st = circuits.layered_z64(n_mul=1_000_000, recycle=True)
        chunk = 1 << 16
        W64 = np.tile(np.asarray(w64, np.uint64), (max(BATCHES), 1))
        W2 = np.zeros((max(BATCHES), 0), np.uint8)
    seeds = rng.integers(0, 256, (max(BATCHES), 256, 16), dtype=np.uint8)
    single_ms, (proof0, info0) = _median_ms(lambda: prove_streaming(prog, W2[0], W64[0], wc, seeds=seeds[0], max_chunk_ops=chunk, ctx=ctx))
    want0 = bytes(proof0)
    del proof0
    rec = {"config": config, "gates": int(st.get("gates", len(prog))), "chunk_ops": chunk, "wire_counts": list(wc),
           "single_stream": {"ms": single_ms, "device_bytes": _device_bytes(info0), "chunks": info0["chunks"]}, "batches": []}
    for B in BATCHES:
        info = {}

        def run():
            info.clear()
            return prove_streaming_batch(prog, W2[:B], W64[:B], wc, seeds=seeds[:B], max_chunk_ops=chunk, ctx=ctx, info=info)

        ms, proofs = _median_ms(run)
        same0 = bytes(proofs[0]) == want0
        del proofs
        rec["batches"].append({"batch": B, "ms_per_call": ms, "ms_per_proof": ms / B, "single_streams_ms": B * single_ms,
                               "speedup_vs_single_streams": B * single_ms / ms, "device_bytes": _device_bytes(info),
                               "proof0_equals_single_stream": same0})
    return rec


def main():
    if len(sys.argv) > 2 and sys.argv[1] == "--step":
        print(json.dumps(step(int(sys.argv[2]))), flush=True)
        return
    me = os.path.abspath(__file__)
    # each GPU step under a time limit of its own, chained: a step that fails, faults or times out ends the run
    cmd = " && ".join(f"timeout -k 10 900 {sys.executable} {me} --step {c}" for c in (4, 5))
    sys.exit(subprocess.call(["bash", "-c", cmd]))


if __name__ == "__main__":
    main()
