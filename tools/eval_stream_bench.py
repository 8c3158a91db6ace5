"""Streaming cleartext evaluation (rv_evaluate_streaming) against the resident path (cold compile + rv_evaluate_batch).

    python tools/eval_stream_bench.py [--reps 5] [--chunks 16,18,20] [--json out.json]

Cases: config4 (the 10^7-gate benchmark circuit, tests/circuits.layered_gf2(): one wire index per gate) and config4r (the same gates
with recycled wire indices, layered_gf2(recycle=True), as a circuit written for streaming numbers them) at B = 1 and 1024, SHA-256
(tests/bristol_gen.py) at B = 1024.  Per case, median of --reps calls, wall time host bytes to host status (no wire values):
  resident_cold_ms   Circuit(ops) + evaluate_batch (the compile included: what a caller with an op list pays)
  resident_compile_ms, resident_eval_ms   the two halves (the eval half on a compiled circuit: GPU-bound)
  stream_ms[2^k]     evaluate_streaming with max_chunk_ops = 2^k (compile on worker threads overlapped with the chunks' GPU work)
  bytes: the stream's wire_store_bytes + peak_chunk_bytes against the resident circuit's device_bytes + its value rows.
The streamed results are checked against the resident ones first."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import reverie_amd  # noqa: E402
from reverie_amd import bristol  # noqa: E402

import bristol_gen  # noqa: E402
import circuits  # noqa: E402


def median_ms(fn, reps):
    fn()  # (warm-up: first-use allocations)
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ts))


def case(name, prog, wc, w2, chunks, reps):
    B = w2.shape[0]
    w64 = np.zeros((B, 0), np.uint64)
    c = reverie_amd.Circuit(prog, wc)
    res = c.evaluate_batch(w2, w64)
    out = {"ops": len(prog), "batch": B, "levels": c.info["levels"]}
    out["resident_compile_ms"] = median_ms(lambda: reverie_amd.Circuit(prog, wc), reps)
    out["resident_eval_ms"] = median_ms(lambda: c.evaluate_batch(w2, w64), reps)
    out["resident_cold_ms"] = median_ms(lambda: reverie_amd.Circuit(prog, wc).evaluate_batch(w2, w64), reps)
    out["resident_bytes"] = int(c.info["device_bytes"] + c.info["gf2_rows_written"] * ((B + 31) // 32) * 4)
    out["resident_scratch_bytes"] = int(c.info["scratch_bytes"])
    out["stream"] = {}
    for k in chunks:
        info = {}
        r = reverie_amd.evaluate_streaming(prog, w2, w64, wc, max_chunk_ops=1 << k, info=info)
        assert np.array_equal(r.n_failed, res.n_failed) and np.array_equal(r.first_failed_op, res.first_failed_op), (name, k)
        ms = median_ms(lambda: reverie_amd.evaluate_streaming(prog, w2, w64, wc, max_chunk_ops=1 << k), reps)
        out["stream"]["2^%d" % k] = {"ms": ms, "chunks": info["chunks"], "wire_store_bytes": info["wire_store_bytes"],
                                     "peak_chunk_bytes": info["peak_chunk_bytes"],
                                     "device_bytes": info["wire_store_bytes"] + info["peak_chunk_bytes"]}
    print(name, json.dumps(out), flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--chunks", default="16,18,20")
    ap.add_argument("--json")
    a = ap.parse_args()
    chunks = [int(x) for x in a.chunks.split(",")]
    rng = np.random.default_rng(1)
    res = {}
    for name, recycle in (("config4", False), ("config4r", True)):
        prog, wit, wc, _st = circuits.layered_gf2(recycle=recycle)
        for B in (1, 1024):
            w2 = rng.integers(0, 2, (B, len(wit))).astype(np.uint8)
            w2[0] = wit
            res["%s_B%d" % (name, B)] = case("%s_B%d" % (name, B), prog, wc, w2, chunks, a.reps)
    sprog, info = bristol.parse(bristol_gen.sha256_block())
    w2 = rng.integers(0, 2, (1024, info["n_inputs"])).astype(np.uint8)
    res["sha256_B1024"] = case("sha256_B1024", sprog, info["wire_counts"], w2, chunks, a.reps)
    if a.json:
        with open(a.json, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
