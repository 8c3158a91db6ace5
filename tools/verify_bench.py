#!/usr/bin/env python3
"""Prover / verifier wall times through the host-bytes entry points (rv_prove / rv_verify, PCIe included)
for the headline circuit and its all-AND variant.  Prints one JSON line per variant.

--proof {host,device,sections} (repeatable; all in one process, on the same circuit and proof) adds "verify_modes" to the line:
the verifier's wall time per call with the proof where that mode has it --
    host      rv_verify_ex on the library's page-locked proof buffer (the README's rv_verify row)
    device    rv_verify_device on the same bytes in a torch GPU tensor
    sections  rv_verify_sections_device on what rv_prove_device left in GPU memory
as median, min and max over --calls calls after --warmup calls, with the calls that took the device path and the proof bytes
the verifier uploaded (rv_hook_verify_device_paths, rv_hook_verify_proof_bytes).  --only-headline leaves the all-AND variant out.

--batch N (with --proof host and / or device; --circuit aes128, sha256 or mixed, repeatable) times the batch entry points instead,
N proofs per call, all modes in one process on the same statements, one JSON line per circuit:
    host      rv_prove_batch, and rv_verify_batch on its proofs
    device    rv_prove_batch_device, and rv_verify_batch_device on what it left in GPU memory
each as median, min and max ms per call (and the median per proof) over --calls calls after --warmup, with the ways the device
verifier's proofs went (rv_hook_verify_batch_device_paths).  The device prover's bytes are compared with the host prover's first.
--witness {host,device} (repeatable, default host; all in one process on the same statements): where the provers take their
witnesses from -- device: torch GPU tensors, read where they lie (rv_prove_batch_wdev / rv_prove_batch_device_wdev), reported as
"prove": {"host_wdev": ..., "device_wdev": ...} beside the host-witness figures."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402

import circuits  # noqa: E402
import reverie_amd  # noqa: E402

ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
ap.add_argument("--proof", action="append", choices=("host", "device", "sections"), default=[],
                help="also time the verifier with the proof in host memory / in a GPU tensor / as rv_prove_device's sections")
ap.add_argument("--calls", type=int, default=9, help="timed calls per --proof mode (median, min, max)")
ap.add_argument("--warmup", type=int, default=2, help="untimed calls per --proof mode")
ap.add_argument("--batch", type=int, default=0, help="time the batch entry points at this many proofs per call instead")
ap.add_argument("--circuit", action="append", choices=("aes128", "sha256", "mixed"), default=[],
                help="--batch: the circuit (default aes128); mixed: the 2 000-gate mixed circuit of tools/batch_z64.py")
ap.add_argument("--witness", action="append", choices=("host", "device"), default=[],
                help="--batch: the provers' witnesses in host memory (default) / in GPU tensors")
ap.add_argument("--only-headline", action="store_true", help="the headline circuit only (p_and = 0.5)")
args = ap.parse_args()


def verify_modes(c, wit, proof):
    """wall times of args.proof's verifier calls on `proof` (a Proof in the library's buffer)"""
    import ctypes as C

    import torch

    from reverie_amd import _lib

    L = _lib.lib()

    def counters():
        out = (C.c_uint64 * 2)()
        L.rv_hook_verify_device_paths(out)
        return int(out[0]), int(L.rv_hook_verify_proof_bytes())

    out = {}
    for mode in args.proof:
        if mode == "host":
            target = proof
        elif mode == "device":
            target = reverie_amd.DeviceProof(torch.frombuffer(bytearray(bytes(proof)), dtype=torch.uint8).cuda())
        else:
            target = reverie_amd.DeviceProof.new(c, wit, [], seeds=seeds)
        ok = all(target.verify(c) for _ in range(args.warmup))
        d0, b0 = counters()
        ts = []
        for _ in range(args.calls):
            t0 = time.perf_counter()
            ok = target.verify(c) and ok
            ts.append((time.perf_counter() - t0) * 1e3)
        d1, b1 = counters()
        out[mode] = {"median_ms": round(statistics.median(ts), 4), "min_ms": round(min(ts), 4), "max_ms": round(max(ts), 4), "calls": args.calls,
                     "ok": bool(ok), "device_path_calls": d1 - d0, "proof_bytes_uploaded": b1 - b0}
    return out


def batch_modes(name, B):
    """the batch entry points on B statements of one circuit: {"prove": {mode: ...}, "verify": {mode: ...}}"""
    import ctypes as C

    from reverie_amd import _lib

    L = _lib.lib()
    if name == "mixed":
        import z64_batch_circuits as zc

        prog, w2, w64, wc = zc.mixed(5, n_gates=2000)
    else:
        import bench

        prog, w2, wc, _ = bench.bristol_case(name)
        w64 = []
    c = reverie_amd.Circuit(prog, wc, whole_prover=True)
    bs = np.random.default_rng(B).integers(0, 256, (B, 256, 16), dtype=np.uint8)
    g = np.tile(np.asarray(w2, np.uint8).reshape(1, -1), (B, 1))
    z = np.tile(np.asarray(w64, np.uint64).reshape(1, -1), (B, 1))
    zz = z if z.shape[1] else None

    def paths():
        out = (C.c_uint64 * 3)()
        L.rv_hook_verify_batch_device_paths(out)
        return [int(x) for x in out]

    def timed(fn):
        for _ in range(args.warmup):
            fn()
        ts = []
        for _ in range(args.calls):
            t0 = time.perf_counter()
            r = fn()
            ts.append((time.perf_counter() - t0) * 1e3)
        med = statistics.median(ts)
        return r, {"median_ms": round(med, 4), "min_ms": round(min(ts), 4), "max_ms": round(max(ts), 4), "ms_per_proof": round(med / B, 5),
                   "calls": args.calls}

    host = reverie_amd.Proof.new_batch(c, g, zz, seeds=bs)
    dev = reverie_amd.prove_batch_device(c, g, zz, seeds=bs)
    if [bytes(p) for p in host] != [d.tensor.cpu().numpy().tobytes() for d in dev]:
        raise SystemExit(f"{name}: rv_prove_batch_device's bytes differ from rv_prove_batch's")
    out = {"circuit": name, "batch": B, "proof_bytes": len(host[0]), "prove": {}, "verify": {}}
    wits = {"host": (g, zz)}
    if "device" in args.witness:
        import torch

        wits["device"] = (torch.from_numpy(g).cuda(), torch.from_numpy(z.view(np.int64)).cuda() if z.shape[1] else None)
        if [bytes(p) for p in reverie_amd.Proof.new_batch(c, *wits["device"], seeds=bs)] != [bytes(p) for p in host]:
            raise SystemExit(f"{name}: rv_prove_batch_wdev's bytes differ from rv_prove_batch's")
    for mode in args.proof:
        if mode == "sections":
            raise SystemExit("--batch takes --proof host and --proof device")
        prover = reverie_amd.Proof.new_batch if mode == "host" else reverie_amd.prove_batch_device
        for where in args.witness or ["host"]:
            wg, wz = wits[where]
            _, out["prove"][mode if where == "host" else mode + "_wdev"] = timed(lambda: prover(c, wg, wz, seeds=bs))
        if mode == "host":
            ok, out["verify"][mode] = timed(lambda: reverie_amd.verify_batch(c, host))
        else:
            p0 = paths()
            ok, out["verify"][mode] = timed(lambda: reverie_amd.verify_batch_device(c, dev))
            out["verify"][mode]["paths"] = [a - b for a, b in zip(paths(), p0)]
        out["verify"][mode]["ok"] = all(ok)
    c.close()
    return out


if args.batch:
    for name in args.circuit or ["aes128"]:
        print(json.dumps(batch_modes(name, args.batch)), flush=True)
    sys.exit(0)

seeds = np.random.default_rng(1).integers(0, 256, (256, 16), dtype=np.uint8)
for p_and in (0.5,) if args.only_headline else (0.5, 1.0):
    prog, wit, wc, st = circuits.layered_gf2(p_and=p_and)
    c = reverie_amd.Circuit(prog, wc)
    proof = reverie_amd.Proof.new(c, wit, [], seeds=seeds)
    t = []
    for _ in range(3):
        t0 = time.perf_counter(); proof = reverie_amd.Proof.new(c, wit, [], seeds=seeds); t.append(time.perf_counter() - t0)
    import ctypes as C

    from reverie_amd import _lib

    def phases(fn, n=3):
        """wall times + the library's own HIP-event phase times (device side only) over n calls"""
        L = _lib.lib()
        L.rv_ctx_profile(c.ctx.handle, 1, 1, None)
        ts = []
        for _ in range(n):
            t0 = time.perf_counter(); r = fn(); ts.append(time.perf_counter() - t0)
        prof = _lib.Profile()
        L.rv_ctx_profile(c.ctx.handle, 0, 0, C.byref(prof))
        return ts, r, {nm: round(prof.ms[i] / n, 3) for i, nm in enumerate(_lib.PHASES)}

    t, proof, prove_phases = phases(lambda: reverie_amd.Proof.new(c, wit, [], seeds=seeds))
    v, ok, verify_phases = phases(lambda: proof.verify(c))
    copy = reverie_amd.Proof(bytes(proof))  # ordinary pageable memory, as a proof read from disk would be
    vp, okp, _ = phases(lambda: copy.verify(c))
    ok = ok and okp
    line = {"p_and": p_and, "and": st["and"], "gates": st["gates"], "proof_bytes": len(proof), "prove_ms_host": min(t) * 1e3,
            "verify_ms_host": min(v) * 1e3, "verify_ms_host_pageable_input": min(vp) * 1e3, "prove_and_per_s_host": st["and"] / min(t), "verify_and_per_s_host": st["and"] / min(v),
            "verify_ok": ok, "prove_device_phases_ms": prove_phases, "verify_device_phases_ms": verify_phases}
    if args.proof:
        line["verify_modes"] = verify_modes(c, wit, proof)
    print(json.dumps(line))
    c.close()
