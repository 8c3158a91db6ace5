"""Cleartext evaluation (rv_evaluate / rv_evaluate_batch) against the host loop of the CLI's `oneshot`.

    python tools/eval_bench.py [--batches 1,64,1024,4096] [--reps 5] [--no-host] [--json out.json]
                               [--witness {host,device}] [--select N] [--config4-batch B] [--only-config4]

config4: the 10^7-gate benchmark circuit (tests/circuits.layered_gf2()), one witness, with and without the wire vector, and the host
evaluator (`reverie_amd.__main__.evaluate_clear`) on it as the baseline.  aes128 / sha256: the Bristol circuits of
tests/bristol_gen.py, evaluate_batch at each batch size: gate x witness per second and microseconds per witness (median of --reps
calls, wall time host bytes to host bytes).  Batched results are checked against single calls first.

--witness device times rv_evaluate_batch_device instead (Circuit.evaluate_batch_device): the witnesses are torch GPU tensors, the
statuses and the values of the first --select GF(2) wires stay in GPU memory (--select 0: statuses only) -- wall time device bytes
to device bytes, checked against the host call first.  --config4-batch B evaluates the benchmark circuit on B copies of its
witness (host witnesses: with the full wire vectors only when they fit --values-gib of host memory).  Every figure comes with its
range: "<key>_range" = [min, max] of the --reps calls."""
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


def timed_ms(fn, reps):
    """(median, [min, max]) of reps calls, ms"""
    fn()  # (warm-up: first-use allocations)
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ts)), [float(min(ts)), float(max(ts))]


def median_ms(fn, reps):
    return timed_ms(fn, reps)[0]


def device_rows(c, w, select, reps):
    """rv_evaluate_batch_device on the witnesses w ([B][n] uint8, host): {"ms", "ms_range"}, the statuses (and the selected
    columns, where the circuit keeps its wires) checked against the host call first"""
    import torch

    tw = torch.from_numpy(np.ascontiguousarray(w)).cuda()
    sel = list(range(select)) if select else None
    r = c.evaluate_batch_device(tw, None, gf2_wires=sel)
    ref = c.evaluate_batch(w, values=bool(select) and w.shape[0] * c.wire_counts[1] <= 1 << 28)
    assert np.array_equal(r.n_failed.cpu().numpy(), ref.n_failed) and np.array_equal(r.first_failed_op.cpu().numpy(), ref.first_failed_op)
    if select and ref.gf2 is not None:
        assert np.array_equal(r.gf2.cpu().numpy(), ref.gf2[:, :select])
    ms, rng = timed_ms(lambda: c.evaluate_batch_device(tw, None, gf2_wires=sel), reps)
    return {"ms": ms, "ms_range": rng}


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
    ap.add_argument("--witness", choices=("host", "device"), default="host", help="device: rv_evaluate_batch_device on GPU tensors")
    ap.add_argument("--select", type=int, default=0, help="--witness device: values of the first N GF(2) wires (0: statuses only)")
    ap.add_argument("--config4-batch", type=int, default=1, help="witnesses per call on the benchmark circuit")
    ap.add_argument("--values-gib", type=float, default=4.0, help="host witnesses: largest wire-vector result to time")
    ap.add_argument("--only-config4", action="store_true")
    a = ap.parse_args()
    res = {}
    prog, wit, wc, st = circuits.layered_gf2()
    c = reverie_amd.Circuit(prog, wc, keep_wires=True)
    n_gates = len(prog)
    assert c.evaluate(wit).ok
    s0 = schedules()
    B4 = a.config4_batch
    w4 = np.tile(np.asarray(wit, np.uint8)[None], (B4, 1))
    res["config4"] = {"ops": n_gates, "levels": c.info["levels"], "B": B4, "witness": a.witness}
    if a.witness == "device":
        res["config4"]["select"] = a.select
        res["config4"].update(device_rows(c, w4, a.select, a.reps))
    else:
        res["config4"]["ms_no_values"], res["config4"]["ms_no_values_range"] = timed_ms(lambda: c.evaluate_batch(w4), a.reps)
        if B4 * wc[1] <= a.values_gib * (1 << 30):
            res["config4"]["ms_values"], res["config4"]["ms_values_range"] = timed_ms(
                (lambda: c.evaluate(wit)) if B4 == 1 else (lambda: c.evaluate_batch(w4, values=True)), a.reps)
    s1 = schedules()
    res["config4"]["schedule"] = "level" if s1[0] > s0[0] else "walk"
    if not a.no_host:
        from reverie_amd.__main__ import evaluate_clear

        t0 = time.perf_counter()
        evaluate_clear(prog, wit)
        res["config4"]["host_ms"] = (time.perf_counter() - t0) * 1e3
    print(json.dumps({"config4": res["config4"]}), flush=True)
    if a.only_config4:
        if a.json:
            with open(a.json, "w") as f:
                json.dump(res, f, indent=1)
        return
    rng = np.random.default_rng(1)
    for name, text, n_in in (("aes128", bristol_gen.aes128(), 256), ("sha256", bristol_gen.sha256_block(), 512)):
        p, info = bristol.parse(text)
        cc = reverie_amd.Circuit(p, info["wire_counts"], keep_wires=a.witness == "device" and a.select > 0)
        n = info["n_gates"]
        rows = []
        for B in [int(x) for x in a.batches.split(",")]:
            w = rng.integers(0, 2, (B, n_in)).astype(np.uint8)
            r = cc.evaluate_batch(w)
            one = cc.evaluate(w[B - 1])
            assert bool(r.ok[B - 1]) == one.ok
            s0 = schedules()
            if a.witness == "device":
                d = device_rows(cc, w, a.select, a.reps)
                ms, ms_range = d["ms"], d["ms_range"]
            else:
                ms, ms_range = timed_ms(lambda: cc.evaluate_batch(w), a.reps)
            s1 = schedules()
            rows.append({"B": B, "ms": ms, "ms_range": ms_range, "witness": a.witness, "select": a.select if a.witness == "device" else None, "us_per_witness": ms * 1e3 / B, "gate_witness_per_s": n * B / (ms * 1e-3),
                         "schedule": "level" if s1[0] > s0[0] else "walk"})
            print(json.dumps({name: rows[-1]}), flush=True)
        res[name] = {"gates": n, "levels": cc.info["levels"], "batches": rows}
    if a.json:
        with open(a.json, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
