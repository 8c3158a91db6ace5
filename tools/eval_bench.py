"""Cleartext evaluation (rv_evaluate / rv_evaluate_batch) against the host loop of the CLI's `oneshot`.

    python tools/eval_bench.py [--batches 1,64,1024,4096] [--reps 5] [--no-host] [--json out.json]

config4: the 10^7-gate benchmark circuit (tests/circuits.layered_gf2()), one witness, with and without the wire vector, and the host
evaluator (`reverie_amd.__main__.evaluate_clear`) on it as the baseline.  aes128 / sha256: the Bristol circuits of
tests/bristol_gen.py, evaluate_batch at each batch size: gate x witness per second and microseconds per witness (median of --reps
calls, wall time host bytes to host bytes).  Batched results are checked against single calls first."""
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
from reverie_amd import _lib, bristol  # noqa: E402

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


def schedules():
    import ctypes as C

    out = (C.c_uint64 * 2)()
    _lib.check(_lib.lib().rv_hook_eval_schedules(out))
    return int(out[0]), int(out[1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="1,64,1024,4096")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--no-host", action="store_true")
    ap.add_argument("--json")
    a = ap.parse_args()
    res = {}
    prog, wit, wc, st = circuits.layered_gf2()
    c = reverie_amd.Circuit(prog, wc, keep_wires=True)
    n_gates = len(prog)
    assert c.evaluate(wit).ok
    s0 = schedules()
    res["config4"] = {"ops": n_gates, "levels": c.info["levels"],
                      "ms_no_values": median_ms(lambda: c.evaluate_batch(np.asarray(wit, np.uint8)[None]), a.reps),
                      "ms_values": median_ms(lambda: c.evaluate(wit), a.reps)}
    s1 = schedules()
    res["config4"]["schedule"] = "level" if s1[0] > s0[0] else "walk"
    if not a.no_host:
        from reverie_amd.__main__ import evaluate_clear

        t0 = time.perf_counter()
        evaluate_clear(prog, wit)
        res["config4"]["host_ms"] = (time.perf_counter() - t0) * 1e3
    print(json.dumps({"config4": res["config4"]}), flush=True)
    rng = np.random.default_rng(1)
    for name, text, n_in in (("aes128", bristol_gen.aes128(), 256), ("sha256", bristol_gen.sha256_block(), 512)):
        p, info = bristol.parse(text)
        cc = reverie_amd.Circuit(p, info["wire_counts"])
        n = info["n_gates"]
        rows = []
        for B in [int(x) for x in a.batches.split(",")]:
            w = rng.integers(0, 2, (B, n_in)).astype(np.uint8)
            r = cc.evaluate_batch(w)
            one = cc.evaluate(w[B - 1])
            assert bool(r.ok[B - 1]) == one.ok
            s0 = schedules()
            ms = median_ms(lambda: cc.evaluate_batch(w), a.reps)
            s1 = schedules()
            rows.append({"B": B, "ms": ms, "us_per_witness": ms * 1e3 / B, "gate_witness_per_s": n * B / (ms * 1e-3),
                         "schedule": "level" if s1[0] > s0[0] else "walk"})
            print(json.dumps({name: rows[-1]}), flush=True)
        res[name] = {"gates": n, "levels": cc.info["levels"], "batches": rows}
    if a.json:
        with open(a.json, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
