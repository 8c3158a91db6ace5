"""Cold compiles of the 10^7-gate benchmark circuit (config 4) and its all-AND variant, host compiler against the device compiler
(RV_COMPILE_DEVICE), in one process on one GPU: rv_circuit_compile_ex wall time (compile + upload, the compiled circuit resident in
HBM), the library's own compile_us / upload_us, the device compiler's per-phase laps (HIP events), and rv_prove_ops with and
without the context flag: cold (the ops cache cleared before the call) and once more on the same ops (from the ops cache).
Medians of `reps` runs after a warm-up, with [min, max] beside them.  --whole-prover: the same table with RV_COMPILE_WHOLE_PROVER
on both compilers (the lazy-sum form).  --compiler device-z64: instead config 5 (circuits.layered_z64) and a half-and-half mixture of
configs 4 and 5 at about 10^6 ops each, host compile + upload against the device compile under RV_COMPILE_DEVICE |
RV_COMPILE_DEVICE_Z64, with the laps (z64: the split of the list and the Z64 ops' steps; the others: the GF(2) ops').
--compiler device-b2a: that mixture with a band of B2A_OPS (default 4096) B2A ops behind it (tools/b2a_workload.py), host compile
against the device compile under RV_COMPILE_DEVICE | RV_COMPILE_DEVICE_Z64 | RV_COMPILE_DEVICE_B2A; MIX_MULS (default 500000) sizes
the mixture.  The host compiler of such a program is the sequential one.
--keep-wires: every compile with RV_COMPILE_KEEP_WIRES, the device's with RV_COMPILE_DEVICE_KEEP_WIRES beside it (without that bit the
flag sends the program to the host compiler); laps_nokeep_ms are the laps of the same device compile without the two flags, so the
difference of the two lap records is the device time of the liveness and wire-table steps.  The rv_prove_ops rows are left out
(rv_prove_ops does not keep wires).
usage: python tools/compile_device_bench.py [--whole-prover] [--keep-wires] [--compiler device|device-z64|device-b2a] [reps]"""
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402

import circuits  # noqa: E402
import reverie_amd  # noqa: E402
from reverie_amd import _lib  # noqa: E402

L = _lib.lib()
args = [a for a in sys.argv[1:] if a not in ("--whole-prover", "--keep-wires")]
COMPILER = "device"
if "--compiler" in args:
    COMPILER = args[args.index("--compiler") + 1]
    assert COMPILER in ("device", "device-z64", "device-b2a"), COMPILER
    del args[args.index("--compiler"):args.index("--compiler") + 2]
WP = _lib.RV_COMPILE_WHOLE_PROVER if "--whole-prover" in sys.argv[1:] else 0
DEV = _lib.RV_COMPILE_DEVICE | (_lib.RV_COMPILE_DEVICE_Z64 if COMPILER != "device" else 0) | (_lib.RV_COMPILE_DEVICE_B2A if COMPILER == "device-b2a" else 0)
KEEP = _lib.RV_COMPILE_KEEP_WIRES if "--keep-wires" in sys.argv[1:] else 0  # (both compilers)
DKEEP = KEEP | (_lib.RV_COMPILE_DEVICE_KEEP_WIRES if KEEP else 0)            # (the device compiler)
reps = int(args[0]) if args else 3
ctx = reverie_amd.Context(0)
seeds = np.arange(4096, dtype=np.uint32).astype(np.uint8).reshape(256, 16)
out = {}


def compile_ms(prog, wc, flags):
    h = C.c_void_p()
    t = time.perf_counter()
    rc = L.rv_circuit_compile_ex(ctx.handle, prog.ctypes.data_as(C.c_void_p), C.c_size_t(len(prog)), C.c_size_t(wc[0]), C.c_size_t(wc[1]),
                                 C.c_uint32(flags), C.byref(h))
    ms = (time.perf_counter() - t) * 1e3
    assert rc == 0, rc
    ci = _lib.CircuitInfo()
    L.rv_circuit_get_info(h, C.byref(ci))
    L.rv_circuit_destroy(h)
    return ms, ci.compile_us / 1e3, ci.upload_us / 1e3


def prove_ops_ms(prog, wit, wc, flags):
    """-> (cold ms, second-call ms, proof bytes)"""
    L.rv_ctx_set_compile_flags(ctx.handle, C.c_uint32(flags))
    L.rv_ctx_ops_cache_clear(ctx.handle)
    ms = []
    for _ in range(2):
        t = time.perf_counter()
        p = reverie_amd.Proof.new(prog, wit, [], wc, seeds=seeds, ctx=ctx)
        ms.append((time.perf_counter() - t) * 1e3)
    L.rv_ctx_set_compile_flags(ctx.handle, C.c_uint32(0))
    return ms[0], ms[1], bytes(p)


LAP_NAMES = ("classify", "writers", "levels", "tables", "download", "rounds")


def device_laps(z64):
    laps, z = (C.c_double * 6)(), C.c_double()
    L.rv_hook_compile_device_laps(laps)
    d = dict(zip(LAP_NAMES, [round(x, 3) for x in laps]))
    if z64:
        L.rv_hook_compile_device_laps_z64(C.byref(z))
        d["z64"] = round(z.value, 3)
    return d


def med(v):
    """median [min, max]"""
    v = np.asarray(v, float)
    return [round(float(np.median(v)), 2), round(float(v.min()), 2), round(float(v.max()), 2)]


def z64_rows():
    """config 5 and the mixture: medians of `reps` cold compiles after one warm-up"""
    p5, w5, wc5, _ = circuits.layered_z64(n_mul=500_000)
    yield "config5", p5, wc5
    p4, _, wc4, _ = circuits.layered_gf2(layers=max(1, len(p5) // 65536))
    n = min(len(p4), len(p5))
    mix = np.empty(2 * n, p5.dtype)  # alternating runs of 4096 ops of each (the domains share no wire)
    run = 4096
    a4 = a5 = at = 0
    while at < 2 * n:
        k = min(run, n - a4)
        mix[at:at + k] = p4[a4:a4 + k]
        at, a4 = at + k, a4 + k
        k = min(run, n - a5)
        mix[at:at + k] = p5[a5:a5 + k]
        at, a5 = at + k, a5 + k
    yield "mix_config4_config5", mix, (wc5[0], wc4[1])


def b2a_rows():
    import b2a_workload

    n_b2a = int(os.environ.get("B2A_OPS", "4096"))
    prog, _, _, wc = b2a_workload.mixed_b2a(n_b2a, int(os.environ.get("MIX_MULS", "500000")))
    yield "mix_config4_config5_b2a%d" % n_b2a, prog, wc


if COMPILER != "device":
    for name, prog, wc in (z64_rows() if COMPILER == "device-z64" else b2a_rows()):
        path, diff = C.c_int(), C.c_int()
        assert L.rv_hook_compile_compare_device(ctx.handle, prog.ctypes.data_as(C.c_void_p), C.c_size_t(len(prog)), C.c_size_t(wc[0]),
                                                C.c_size_t(wc[1]), C.c_uint32(WP | DEV | DKEEP), C.byref(path), C.byref(diff)) == 0
        rec = {"ops": len(prog), "whole_prover": bool(WP), "keep_wires": bool(KEEP), "device_path": path.value, "diff": diff.value, "host": [],
               "device": [], "laps_ms": []}
        compile_ms(prog, wc, WP | KEEP)
        compile_ms(prog, wc, WP | DEV | DKEEP)
        for _ in range(reps):
            rec["host"].append(compile_ms(prog, wc, WP | KEEP))
            rec["device"].append(compile_ms(prog, wc, WP | DEV | DKEEP))
            rec["laps_ms"].append(device_laps(True))
            if KEEP:
                compile_ms(prog, wc, WP | DEV)
                rec.setdefault("laps_nokeep_ms", []).append(device_laps(True))
        for k in ("host", "device"):
            v = np.array(rec[k])
            rec[k + "_ms"] = {"wall": med(v[:, 0]), "compile": med(v[:, 1]), "upload": med(v[:, 2])}
            del rec[k]
        print(name, json.dumps(rec), flush=True)
    ctx.close()
    sys.exit(0)

for name, p_and in (("config4", 0.5), ("all_and", 1.0)):
    prog, wit, wc, st = circuits.layered_gf2(p_and=p_and)
    wit = list(wit)
    path, diff = C.c_int(), C.c_int()
    assert L.rv_hook_compile_compare_device(ctx.handle, prog.ctypes.data_as(C.c_void_p), C.c_size_t(len(prog)), C.c_size_t(wc[0]),
                                            C.c_size_t(wc[1]), C.c_uint32(WP | DEV | DKEEP if WP or KEEP else 0), C.byref(path), C.byref(diff)) == 0
    rec = {"ops": len(prog), "whole_prover": bool(WP), "keep_wires": bool(KEEP), "device_path": path.value, "diff": diff.value, "host": [],
           "device": [], "laps_ms": []}
    compile_ms(prog, wc, WP | KEEP)  # (warm-up: the arena's blocks, the page-locked staging buffer)
    compile_ms(prog, wc, WP | DEV | DKEEP)
    for _ in range(reps):
        rec["host"].append(compile_ms(prog, wc, WP | KEEP))
        rec["device"].append(compile_ms(prog, wc, WP | DEV | DKEEP))
        rec["laps_ms"].append(device_laps(False))
        if KEEP:
            compile_ms(prog, wc, WP | DEV)
            rec.setdefault("laps_nokeep_ms", []).append(device_laps(False))
    # rv_prove_ops chooses its own form (the context flag decides where it is compiled): the same rows with and without --whole-prover
    if not KEEP:
        prove_ops_ms(prog, wit, wc, 0)
        runs = {"host": [], "device": []}
        same = True
        for _ in range(reps):
            h = prove_ops_ms(prog, wit, wc, 0)
            d = prove_ops_ms(prog, wit, wc, DEV)
            runs["host"].append(h[:2])
            runs["device"].append(d[:2])
            same = same and h[2] == d[2]
        rec["prove_ops_cold_ms"] = {k: med([r[0] for r in v]) for k, v in runs.items()}
        rec["prove_ops_second_ms"] = {k: med([r[1] for r in v]) for k, v in runs.items()}
        rec["prove_ops_same_bytes"] = same
    for k in ("host", "device"):
        v = np.array(rec[k])
        rec[k + "_ms"] = {"wall": med(v[:, 0]), "compile": med(v[:, 1]), "upload": med(v[:, 2])}
        del rec[k]
    out[name] = rec
    print(name, json.dumps(rec), flush=True)
L.rv_ctx_ops_cache_clear(ctx.handle)
ctx.close()
