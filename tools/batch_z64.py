"""Z64 / mixed circuits: ms per proof of a loop of Proof.new against one Proof.new_batch, and of a loop of Proof.verify against
one verify_batch, at several batch sizes.  Every batched proof is compared with its single proof (and every batched verdict
with the single verifier's) before any time is printed.

    python tools/batch_z64.py [--batches 1,2,8,64,256] [--reps 3] [--circuits chain,mixed,layered] [--json out.json]

chain: 4 lanes of x <- x*x + c for 128 rounds (pure Z64, every level narrow); mixed: circuits.random_mixed with ~2 000 gates
(B2A, Random, SizeHint); layered: circuits.layered_z64 with ~10^4 Mul gates."""
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
import z64_batch_circuits as zc  # noqa: E402


def build(name):
    if name == "chain":
        prog, wit, wc = zc.chain_z64()
        return prog, [], wit, wc
    if name == "mixed":
        prog, w2, w64, wc = zc.mixed(5, n_gates=2000)
        return prog, w2, w64, wc
    if name == "layered":
        prog, wit, wc = zc.layered_small(10_000)
        return prog, [], wit, wc
    raise SystemExit(f"unknown circuit {name}")


def best(fn, reps):
    ts = []
    for _ in range(reps):
        t = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t)
    return min(ts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="1,2,8,64,256")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--circuits", default="chain,mixed,layered")
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    batches = [int(x) for x in a.batches.split(",")]
    bmax = max(batches)
    rows = []
    for name in a.circuits.split(","):
        prog, w2, w64, wc = build(name)
        c = reverie_amd.Circuit(prog, wc, whole_prover=True)
        info = c.info
        rng = np.random.default_rng(1)
        seeds = rng.integers(0, 256, (bmax, 256, 16), dtype=np.uint8)
        g = np.tile(np.asarray(w2, np.uint8).reshape(1, -1), (bmax, 1))
        z = np.tile(np.asarray(w64, np.uint64).reshape(1, -1), (bmax, 1))
        # correctness first: every batched proof against its single proof, every batched verdict against the single verifier's
        singles = [reverie_amd.Proof.new(c, g[b], z[b], seeds=seeds[b]) for b in range(bmax)]
        got = reverie_amd.Proof.new_batch(c, g, z, seeds=seeds)
        for b in range(bmax):
            if bytes(got[b]) != bytes(singles[b]):
                raise SystemExit(f"{name}: batched proof {b} differs from its single proof")
        vs = reverie_amd.verify_batch(c, got)
        if vs != [p.verify(c) for p in singles] or not all(vs):
            raise SystemExit(f"{name}: verify_batch differs from the single verifier")
        del got
        for B in batches:
            t_loop = best(lambda: [reverie_amd.Proof.new(c, g[b], z[b], seeds=seeds[b]) for b in range(B)], a.reps)
            t_batch = best(lambda: reverie_amd.Proof.new_batch(c, g[:B], z[:B], seeds=seeds[:B]), a.reps)
            t_vloop = best(lambda: [singles[b].verify(c) for b in range(B)], a.reps)
            t_vbatch = best(lambda: reverie_amd.verify_batch(c, singles[:B]), a.reps)
            row = {"circuit": name, "ops": int(info["n_ops"]), "levels": int(info["levels"]), "B": B,
                   "prove_loop_ms": 1e3 * t_loop / B, "prove_batch_ms": 1e3 * t_batch / B,
                   "verify_loop_ms": 1e3 * t_vloop / B, "verify_batch_ms": 1e3 * t_vbatch / B}
            rows.append(row)
            print(f"{name:8s} levels {row['levels']:5d}  B {B:4d}  prove loop {row['prove_loop_ms']:8.3f}  batch {row['prove_batch_ms']:8.3f} ms/proof"
                  f"   verify loop {row['verify_loop_ms']:8.3f}  batch {row['verify_batch_ms']:8.3f} ms/proof", flush=True)
        c.close()
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        json.dump(rows, open(a.json, "w"), indent=1)


if __name__ == "__main__":
    main()
