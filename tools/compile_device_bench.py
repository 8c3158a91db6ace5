"""Cold compiles of the 10^7-gate benchmark circuit (config 4) and its all-AND variant, host compiler against the device compiler
(RV_COMPILE_DEVICE), in one process on one GPU: rv_circuit_compile_ex wall time (compile + upload, the compiled circuit resident in
HBM), the library's own compile_us / upload_us, the device compiler's per-phase laps (HIP events), and a cold rv_prove_ops with and
without the context flag (the ops cache cleared before every call).
usage: python tools/compile_device_bench.py [reps]"""
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
reps = int(sys.argv[1]) if len(sys.argv) > 1 else 3
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
    L.rv_ctx_set_compile_flags(ctx.handle, C.c_uint32(flags))
    L.rv_ctx_ops_cache_clear(ctx.handle)
    t = time.perf_counter()
    p = reverie_amd.Proof.new(prog, wit, [], wc, seeds=seeds, ctx=ctx)
    ms = (time.perf_counter() - t) * 1e3
    L.rv_ctx_set_compile_flags(ctx.handle, C.c_uint32(0))
    return ms, bytes(p)


for name, p_and in (("config4", 0.5), ("all_and", 1.0)):
    prog, wit, wc, st = circuits.layered_gf2(p_and=p_and)
    wit = list(wit)
    path, diff = C.c_int(), C.c_int()
    assert L.rv_hook_compile_compare_device(ctx.handle, prog.ctypes.data_as(C.c_void_p), C.c_size_t(len(prog)), C.c_size_t(wc[0]),
                                            C.c_size_t(wc[1]), C.c_uint32(0), C.byref(path), C.byref(diff)) == 0
    rec = {"ops": len(prog), "device_path": path.value, "diff": diff.value, "host": [], "device": [], "laps_ms": []}
    compile_ms(prog, wc, 0)  # (warm-up: the arena's blocks, the page-locked staging buffer)
    compile_ms(prog, wc, 4)
    for _ in range(reps):
        rec["host"].append(compile_ms(prog, wc, 0))
        rec["device"].append(compile_ms(prog, wc, 4))
        laps = (C.c_double * 6)()
        L.rv_hook_compile_device_laps(laps)
        rec["laps_ms"].append(dict(zip(("classify", "writers", "levels", "tables", "download", "rounds"), [round(x, 3) for x in laps])))
    hp, hb = prove_ops_ms(prog, wit, wc, 0)
    dp, db = prove_ops_ms(prog, wit, wc, 4)
    rec["prove_ops_cold_ms"] = {"host": round(hp, 2), "device": round(dp, 2), "same_bytes": hb == db}
    for k in ("host", "device"):
        v = np.array(rec[k])
        rec[k + "_ms"] = {"wall": round(float(np.median(v[:, 0])), 2), "compile": round(float(np.median(v[:, 1])), 2),
                          "upload": round(float(np.median(v[:, 2])), 2)}
        del rec[k]
    out[name] = rec
    print(name, json.dumps(rec), flush=True)
L.rv_ctx_ops_cache_clear(ctx.handle)
ctx.close()
