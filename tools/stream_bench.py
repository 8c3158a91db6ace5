"""Streaming prover on the benchmark workloads: time, device footprint, byte equality with rv_prove.

    python tools/stream_bench.py            # config 4 (recycled wire indices) and config 5
    python tools/stream_bench.py --compiler device            # the same with the pieces compiled on the GPU (RV_COMPILE_DEVICE)
    python tools/stream_bench.py --compiler device-z64 --z64 [--runs 5]   # config 5 (Z64) at the chosen compiler, beside RV_STREAM_THREADS=1
    python tools/stream_bench.py --compare [--runs 5]         # config 4, host and device compiler side by side, one JSON line per row
    python tools/stream_bench.py --compiler device --ops device [--runs 5]   # config 4 fed from a GPU tensor (rv_stream_feed_device) beside
                                                              # the same calls fed from host memory, one JSON line per entry point
    python tools/stream_bench.py --witness device --proof device [--ops device --compiler device] [--runs 5]   # config 4 with the witness
                                                              # in a GPU tensor and / or the proof left in one (rv_stream_feed_wdev,
                                                              # rv_stream_finish_device, rv_stream_verify_begin_device) beside the default
                                                              # host cell, one JSON line per entry point
bench.py imports streaming_record() for its `streaming` record.  RV_STREAM_STATS=1 prints the feeds' laps; with the device compiler they
name the op upload, the device compile and the host copy of the pieces."""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402


def streaming_record(ctx, prog, wit, wc, st, seeds, want: bytes, chunk_ops: int = 1 << 18, layers: int = 153, p_and: float = 0.5):
    """config 4 through rv_prove_streaming.  The circuit is regenerated with recycled wire indices (the proof does not
    depend on wire numbering, the streaming prover's wire store does); `want` = rv_prove's proof of the same statement."""
    import circuits
    from reverie_amd.stream import prove_streaming

    rprog, rwit, rwc, rst = circuits.layered_gf2(layers=layers, p_and=p_and, recycle=True)
    from reverie_amd.stream import verify_streaming

    # median of the five calls after a warm-up (which also sizes the context's staging buffers and starts the worker threads); the
    # record is bound by 24 host threads compiling pieces: 65 - 77 ms in three consecutive bench runs on one box
    dts, tvs = [], []
    for _ in range(6):
        t0 = time.perf_counter()
        proof, info = prove_streaming(rprog, rwit, [], rwc, seeds=seeds, max_chunk_ops=chunk_ops, ctx=ctx)
        dts.append(time.perf_counter() - t0)
        tv = time.perf_counter()
        vok, vinfo = verify_streaming(rprog, rwc, proof, max_chunk_ops=chunk_ops, ctx=ctx)
        tvs.append(time.perf_counter() - tv)
    first_dt, first_tv = dts[0], tvs[0]
    dts, tvs = dts[1:], tvs[1:]
    dt, tv = sorted(dts)[2], sorted(tvs)[2]
    rec = {"value": rst["and"] / dt, "unit": "AND gates/s", "ms": dt * 1e3, "ms_min_max": [min(dts) * 1e3, max(dts) * 1e3], "first_call_ms": first_dt * 1e3, "chunk_ops": chunk_ops, "chunks": info["chunks"],
           "gf2_wires": rwc[1], "bit_exact_vs_rv_prove": bytes(proof) == want,
           "verify_streaming": {"ms": tv * 1e3, "ms_min_max": [min(tvs) * 1e3, max(tvs) * 1e3], "first_call_ms": first_tv * 1e3, "ok": vok, "device_bytes_beside_the_proof": vinfo["wire_store_bytes"] + vinfo["peak_chunk_bytes"] + vinfo["hash_state_bytes"],
                                "note": "rv_verify_streaming (strict): one pass over the op array, chunks in verify mode against the proof"},
           "device_bytes": dict({k: info[k] for k in ("wire_store_bytes", "peak_chunk_bytes", "hash_state_bytes", "proof_bytes")},
                                kept_transcript_bytes=info["kept_mib"] << 20),
           "note": "rv_prove_streaming, host ops in -> host proof bytes out, two passes over the op array; every chunk is compiled "
                   "(levelised) and moved to its transcript offsets on one of up to 24 worker threads ahead of the GPU, and its compiled "
                   "form kept for pass 2 while it fits RV_STREAM_CACHE_MB; pass 1 keeps the last chunks' transcripts on the device within "
                   "RV_STREAM_KEEP_MB (rv_stream_same_cuts; here: all of them, kept_transcript_bytes) and pass 2 takes their openings "
                   "from them instead of running them again; a long feed starts with pieces of 1/8, 1/4 and 1/2 of the chunk size; "
                   "the resident prover keeps ~6.4 GB for this circuit"}
    # the regime the streaming prover exists for: NO transcripts kept between the passes (RV_STREAM_KEEP_MB=0: every chunk runs
    # twice, device memory = wire store + one chunk + the proof), same bytes
    os.environ["RV_STREAM_KEEP_MB"] = "0"
    try:
        bts = []
        for _ in range(4):
            t0 = time.perf_counter()
            bproof, binfo = prove_streaming(rprog, rwit, [], rwc, seeds=seeds, max_chunk_ops=chunk_ops, ctx=ctx)
            bts.append(time.perf_counter() - t0)
        bts = sorted(bts[1:])
        rec["bounded_memory"] = {"ms": bts[1] * 1e3, "ms_min_max": [bts[0] * 1e3, bts[-1] * 1e3], "value": rst["and"] / bts[1], "unit": "AND gates/s",
                                 "bit_exact_vs_rv_prove": bytes(bproof) == want, "kept_transcript_bytes": binfo["kept_mib"] << 20,
                                 "device_bytes": {k: binfo[k] for k in ("wire_store_bytes", "peak_chunk_bytes", "hash_state_bytes", "proof_bytes")},
                                 "note": "RV_STREAM_KEEP_MB=0: pass 2 runs every chunk again (masks, levels, openings); median of 3 after a warm-up"}
        del bproof
    finally:
        os.environ.pop("RV_STREAM_KEEP_MB", None)
    del proof
    return rec


def _timed(f, runs):
    """median and min - max (ms) of `runs` calls after a warm-up, and the last result"""
    out = f()
    dts = []
    for _ in range(runs):
        t0 = time.perf_counter()
        out = f()
        dts.append((time.perf_counter() - t0) * 1e3)
    dts.sort()
    return {"ms": dts[len(dts) // 2], "ms_min_max": [dts[0], dts[-1]]}, out


def compare_compilers(ctx, seeds, want: bytes, runs: int = 5, chunk_ops: int = 1 << 18, layers: int = 153):
    """config 4 (recycled wire indices) through every streaming entry point, pieces compiled on the host (the default) and on the GPU:
    yields one record per row.  The proofs are compared with rv_prove's, the evaluator's values between the two compilers."""
    import circuits
    from reverie_amd import _lib
    from reverie_amd.stream import evaluate_streaming, prove_streaming, prove_streaming_batch, verify_streaming

    prog, wit, wc, st = circuits.layered_gf2(layers=layers, recycle=True)
    wit = np.asarray(wit, np.uint8)
    chunks = _lib.lib().rv_hook_stream_device_chunks
    proof0, _ = prove_streaming(prog, wit, [], wc, seeds=seeds, max_chunk_ops=chunk_ops, ctx=ctx)
    bseeds = np.stack([np.roll(seeds, b, axis=0) for b in range(8)])
    bwits = np.tile(wit, (8, 1))
    values = {}

    def row(name, f, check, env=None):
        for k, v in (env or {}).items():
            os.environ[k] = v
        try:
            rec = {"row": name}
            for compiler in ("host", "device"):
                before = chunks()
                t, out = _timed(lambda: f(compiler == "device"), runs)
                rec[compiler] = dict(t, ok=bool(check(out, compiler)), device_chunks_per_call=(chunks() - before) // (runs + 1))
            rec["device_over_host"] = rec["device"]["ms"] / rec["host"]["ms"]
            return rec
        finally:
            for k in env or {}:
                os.environ.pop(k, None)

    def same_values(out, compiler):
        key = out.gf2.tobytes()
        values.setdefault("host", key)
        return bool(out.ok.all()) and values["host"] == key

    prove = lambda dev: prove_streaming(prog, wit, [], wc, seeds=seeds, max_chunk_ops=chunk_ops, ctx=ctx, device_compile=dev)
    yield row("prove_streaming", prove, lambda o, c: bytes(o[0]) == want)
    yield row("verify_streaming", lambda dev: verify_streaming(prog, wc, proof0, max_chunk_ops=chunk_ops, ctx=ctx, device_compile=dev), lambda o, c: o[0])
    yield row("prove_streaming RV_STREAM_KEEP_MB=0", prove, lambda o, c: bytes(o[0]) == want, {"RV_STREAM_KEEP_MB": "0"})
    yield row("evaluate_streaming", lambda dev: evaluate_streaming(prog, wit, [], wc, max_chunk_ops=chunk_ops, values=True, ctx=ctx, device_compile=dev),
              same_values)
    yield row("prove_streaming_batch of 8",
              lambda dev: prove_streaming_batch(prog, bwits, [], wc, seeds=bseeds, max_chunk_ops=chunk_ops, ctx=ctx, device_compile=dev),
              lambda o, c: bytes(o[0]) == want and len(o) == 8)
    yield row("prove_streaming RV_STREAM_THREADS=1", prove, lambda o, c: bytes(o[0]) == want, {"RV_STREAM_THREADS": "1"})


def device_ops_rows(ctx, seeds, want: bytes, runs: int = 5, chunk_ops: int = 1 << 18, layers: int = 153):
    """config 4 (recycled wire indices) through the prover, verifier and evaluator with the op list in host memory and in a GPU tensor
    (uploaded once, outside the timed region), at the context's compile flags: one record per entry point, with the op bytes each
    call moved (rv_hook_stream_op_traffic: host -> device, device -> host)."""
    import ctypes as C

    import torch

    import circuits
    from reverie_amd import _lib
    from reverie_amd.stream import evaluate_streaming, prove_streaming, verify_streaming

    prog, wit, wc, st = circuits.layered_gf2(layers=layers, recycle=True)
    wit = np.asarray(wit, np.uint8)
    d_prog = torch.from_numpy(prog.view(np.uint8).reshape(-1, prog.dtype.itemsize)).to(f"cuda:{ctx.device}")
    torch.cuda.synchronize()
    proof0, _ = prove_streaming(prog, wit, [], wc, seeds=seeds, max_chunk_ops=chunk_ops, ctx=ctx)
    values = {}

    def traffic():
        out = (C.c_uint64 * 2)()
        _lib.check(_lib.lib().rv_hook_stream_op_traffic(out))
        return np.array([int(out[0]), int(out[1])])

    def same_values(out):
        key = out.gf2.tobytes()
        values.setdefault("first", key)
        return bool(out.ok.all()) and values["first"] == key

    calls = [("prove_streaming", lambda ops: prove_streaming(ops, wit, [], wc, seeds=seeds, max_chunk_ops=chunk_ops, ctx=ctx), lambda o: bytes(o[0]) == want),
             ("verify_streaming", lambda ops: verify_streaming(ops, wc, proof0, max_chunk_ops=chunk_ops, ctx=ctx), lambda o: bool(o[0])),
             ("evaluate_streaming", lambda ops: evaluate_streaming(ops, wit, [], wc, max_chunk_ops=chunk_ops, values=True, ctx=ctx), same_values)]
    for name, f, check in calls:
        rec = {"row": name, "n_ops": int(len(prog)), "chunk_ops": chunk_ops, "compile_flags": int(getattr(ctx, "compile_flags", 0))}
        for where, ops in (("host_ops", prog), ("device_ops", d_prog)):
            before = traffic()
            t, out = _timed(lambda: f(ops), runs)
            rec[where] = dict(t, ok=bool(check(out)), op_bytes_h2d_d2h_per_call=[int(x) for x in (traffic() - before) // (runs + 1)])
        rec["device_over_host"] = rec["device_ops"]["ms"] / rec["host_ops"]["ms"]
        yield rec


def device_memory_rows(ctx, seeds, want: bytes, ops="host", witness="host", proof="host", runs: int = 5, chunk_ops: int = 1 << 18, layers: int = 153):
    """config 4 (recycled wire indices) through prove_streaming with the ops, the witness and the proof each in host memory or in GPU
    memory (tensors uploaded once, outside the timed region), beside the all-host cell, at the context's compile flags; then
    verify_streaming on host proof bytes and -- proof == "device" -- on a DeviceProof.  One record per entry point, with the witness
    and proof bytes each call moved (rv_hook_stream_traffic)."""
    import ctypes as C

    import torch

    import circuits
    from reverie_amd import _lib
    from reverie_amd.stream import prove_streaming, verify_streaming

    prog, wit, wc, st = circuits.layered_gf2(layers=layers, recycle=True)
    wit = np.asarray(wit, np.uint8)
    dev = f"cuda:{ctx.device}"
    d_prog = torch.from_numpy(prog.view(np.uint8).reshape(-1, prog.dtype.itemsize)).to(dev) if ops == "device" else None
    d_wit, d_w64 = torch.from_numpy(wit).to(dev), torch.zeros(0, dtype=torch.int64, device=dev)
    torch.cuda.synchronize()

    def traffic():
        out = (C.c_uint64 * 4)()
        _lib.check(_lib.lib().rv_hook_stream_traffic(out))
        return np.array([int(x) for x in out])

    def host_bytes(p):
        return bytes(p) if proof == "host" else p.tensor.cpu().numpy().tobytes()

    cell = {"ops": ops, "witness": witness, "proof": proof}
    rec = {"row": "prove_streaming", "n_ops": int(len(prog)), "chunk_ops": chunk_ops, "compile_flags": int(getattr(ctx, "compile_flags", 0)), "cell": cell}
    before = traffic()
    t, out = _timed(lambda: prove_streaming(prog, wit, [], wc, seeds=seeds, max_chunk_ops=chunk_ops, ctx=ctx), runs)
    rec["host_cell"] = dict(t, ok=bytes(out[0]) == want, witness_h2d_dev_proof_d2h_h2d_per_call=[int(x) for x in (traffic() - before) // (runs + 1)])
    before = traffic()
    t, out = _timed(lambda: prove_streaming(d_prog if ops == "device" else prog, d_wit if witness == "device" else wit, d_w64 if witness == "device" else [],
                                            wc, seeds=seeds, max_chunk_ops=chunk_ops, ctx=ctx, device_proof=proof == "device"), runs)
    rec["this_cell"] = dict(t, ok=host_bytes(out[0]) == want, witness_h2d_dev_proof_d2h_h2d_per_call=[int(x) for x in (traffic() - before) // (runs + 1)])
    rec["this_over_host"] = rec["this_cell"]["ms"] / rec["host_cell"]["ms"]
    yield rec
    made = out[0]
    rec = {"row": "verify_streaming", "n_ops": int(len(prog)), "chunk_ops": chunk_ops, "cell": cell}
    before = traffic()
    t, vout = _timed(lambda: verify_streaming(prog, wc, want, max_chunk_ops=chunk_ops, ctx=ctx), runs)
    rec["host_cell"] = dict(t, ok=bool(vout[0]), witness_h2d_dev_proof_d2h_h2d_per_call=[int(x) for x in (traffic() - before) // (runs + 1)])
    if proof == "device":
        before = traffic()
        t, vout = _timed(lambda: verify_streaming(d_prog if ops == "device" else prog, wc, made, max_chunk_ops=chunk_ops, ctx=ctx), runs)
        rec["this_cell"] = dict(t, ok=bool(vout[0]), witness_h2d_dev_proof_d2h_h2d_per_call=[int(x) for x in (traffic() - before) // (runs + 1)])
        rec["this_over_host"] = rec["this_cell"]["ms"] / rec["host_cell"]["ms"]
    yield rec


def z64_compiler_rows(ctx, seeds, runs=5, n_mul=1_000_000, chunk_ops=1 << 16):
    """config 5 through prove_streaming at the context's compile flags, with the default worker threads and with RV_STREAM_THREADS=1:
    medians of `runs` calls after a warm-up, the pieces the device compiler took per call, the proof against rv_prove's"""
    import circuits
    import reverie_amd
    from reverie_amd import _lib
    from reverie_amd.stream import prove_streaming

    prog, w64, wc, st = circuits.layered_z64(n_mul=n_mul, recycle=True)
    circ = reverie_amd.Circuit(prog, wc, ctx)
    want = bytes(reverie_amd.Proof.new(circ, [], w64, seeds=seeds))
    circ.close()
    for env in ({}, {"RV_STREAM_THREADS": "1"}):
        os.environ.update(env)
        try:
            before = int(_lib.lib().rv_hook_stream_device_chunks())
            t, out = _timed(lambda: prove_streaming(prog, [], w64, wc, seeds=seeds, max_chunk_ops=chunk_ops, ctx=ctx), runs)
            yield dict(t, row="prove_streaming config 5" + "".join(" %s=%s" % kv for kv in env.items()), n_ops=int(len(prog)), chunk_ops=chunk_ops,
                       compile_flags=int(getattr(ctx, "compile_flags", 0)), ok=bytes(out[0]) == want,
                       device_chunks_per_call=(int(_lib.lib().rv_hook_stream_device_chunks()) - before) // (runs + 1))
        finally:
            for k in env:
                os.environ.pop(k, None)


def b2a_compiler_rows(ctx, seeds, runs=5, n_b2a=4096, n_mul=500_000, chunk_ops=1 << 16):
    """the mixed workload with a band of B2A ops (tools/b2a_workload.py) through prove_streaming at the context's compile flags, as
    z64_compiler_rows"""
    import b2a_workload
    import reverie_amd
    from reverie_amd import _lib
    from reverie_amd.stream import prove_streaming

    prog, w2, w64, wc = b2a_workload.mixed_b2a(n_b2a, n_mul, recycle=True)
    circ = reverie_amd.Circuit(prog, wc, ctx)
    want = bytes(reverie_amd.Proof.new(circ, w2, w64, seeds=seeds))
    circ.close()
    for env in ({}, {"RV_STREAM_THREADS": "1"}):
        os.environ.update(env)
        try:
            before = int(_lib.lib().rv_hook_stream_device_chunks())
            t, out = _timed(lambda: prove_streaming(prog, w2, w64, wc, seeds=seeds, max_chunk_ops=chunk_ops, ctx=ctx), runs)
            yield dict(t, row="prove_streaming mixture + %d B2A" % n_b2a + "".join(" %s=%s" % kv for kv in env.items()), n_ops=int(len(prog)),
                       chunk_ops=chunk_ops, compile_flags=int(getattr(ctx, "compile_flags", 0)), ok=bytes(out[0]) == want,
                       device_chunks_per_call=(int(_lib.lib().rv_hook_stream_device_chunks()) - before) // (runs + 1))
        finally:
            for k in env:
                os.environ.pop(k, None)


def z64_record(ctx, seeds, n_mul=1_000_000, chunk_ops=1 << 16):
    import circuits
    import reverie_amd
    from reverie_amd.stream import prove_streaming

    prog, w64, wc, st = circuits.layered_z64(n_mul=n_mul, recycle=True)  # (wire numbering does not reach the proof)
    dts = []
    for _ in range(3):  # (median of three: the first call sizes the context's buffers)
        t0 = time.perf_counter()
        proof, info = prove_streaming(prog, [], w64, wc, seeds=seeds, max_chunk_ops=chunk_ops, ctx=ctx)
        dts.append(time.perf_counter() - t0)
    dt = sorted(dts)[1]
    from reverie_amd.stream import verify_streaming

    tv = time.perf_counter()
    vok, vinfo = verify_streaming(prog, wc, proof, max_chunk_ops=chunk_ops, ctx=ctx)
    tv = time.perf_counter() - tv
    circ = reverie_amd.Circuit(prog, wc, ctx)
    want = reverie_amd.Proof.new(circ, [], w64, seeds=seeds)
    rec = {"value": st["mul"] / dt, "unit": "Z64 MUL gates/s", "ms": dt * 1e3, "chunk_ops": chunk_ops, "chunks": info["chunks"],
           "verify_streaming": {"ms": tv * 1e3, "ok": vok, "device_bytes_beside_the_proof": vinfo["wire_store_bytes"] + vinfo["peak_chunk_bytes"] + vinfo["hash_state_bytes"]},
           "z64_wires": wc[0], "bit_exact_vs_rv_prove": bytes(proof) == bytes(want), "resident_prover_scratch_bytes": circ.info["scratch_bytes"],
           "device_bytes": dict({k: info[k] for k in ("wire_store_bytes", "peak_chunk_bytes", "hash_state_bytes", "proof_bytes")},
                                kept_transcript_bytes=info["kept_mib"] << 20)}
    circ.close()
    return rec


if __name__ == "__main__":
    import argparse
    import json

    import circuits
    import reverie_amd

    ap = argparse.ArgumentParser()
    ap.add_argument("--compiler", default="host", choices=["host", "device", "device-z64", "device-b2a"],
                    help="where the streams' pieces are compiled (device: RV_COMPILE_DEVICE; device-z64: with RV_COMPILE_DEVICE_Z64, Z64 and mixed pieces too; "
                         "device-b2a: with RV_COMPILE_DEVICE_B2A as well, every piece)")
    ap.add_argument("--b2a", action="store_true",
                    help="the config 4 / config 5 mixture with a band of B2A_OPS (default 4096) B2A ops only: prove_streaming at the chosen compiler, "
                         "default threads and RV_STREAM_THREADS=1")
    ap.add_argument("--z64", action="store_true", help="config 5 only: prove_streaming at the chosen compiler, default threads and RV_STREAM_THREADS=1")
    ap.add_argument("--compare", action="store_true", help="config 4 with both compilers, every streaming entry point")
    ap.add_argument("--ops", default="host", choices=["host", "device"],
                    help="device: config 4 fed from a GPU tensor beside the host-fed calls (prover, verifier, evaluator), one JSON line each")
    ap.add_argument("--witness", default="host", choices=["host", "device"],
                    help="device: config 4 with the witness read from a GPU tensor (rv_stream_feed_wdev) beside the all-host cell")
    ap.add_argument("--proof", default="host", choices=["host", "device"],
                    help="device: config 4 with the proof left in a GPU tensor (rv_stream_finish_device) and verified there "
                         "(rv_stream_verify_begin_device) beside the all-host cell; combines with --witness and --ops")
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--bench-record", action="store_true")
    args = ap.parse_args()
    ctx = reverie_amd.Context(0)
    if args.compiler != "host":  # (the one-shot calls follow the context's flags)
        from reverie_amd import _lib

        ctx.set_compile_flags(_lib.RV_COMPILE_DEVICE | (_lib.RV_COMPILE_DEVICE_Z64 if args.compiler != "device" else 0) |
                              (_lib.RV_COMPILE_DEVICE_B2A if args.compiler == "device-b2a" else 0))
    seeds = np.random.default_rng(0x5EED).integers(0, 256, (256, 16), dtype=np.uint8)
    if args.b2a:
        for rec in b2a_compiler_rows(ctx, seeds, runs=args.runs, n_b2a=int(os.environ.get("B2A_OPS", "4096")), n_mul=int(os.environ.get("MIX_MULS", "500000"))):
            print(json.dumps(rec), flush=True)
        sys.exit(0)
    if args.z64:
        for rec in z64_compiler_rows(ctx, seeds, runs=args.runs, n_mul=int(os.environ.get("Z64_MULS", "1000000"))):
            print(json.dumps(rec), flush=True)
        sys.exit(0)
    layers = int(os.environ.get("LAYERS", "153"))
    prog, wit, wc, st = circuits.layered_gf2(layers=layers)
    circ = reverie_amd.Circuit(prog, wc, ctx)
    want = bytes(reverie_amd.Proof.new(circ, wit, [], seeds=seeds))
    circ.close()
    if args.witness == "device" or args.proof == "device":
        for rec in device_memory_rows(ctx, seeds, want, ops=args.ops, witness=args.witness, proof=args.proof, runs=args.runs, layers=layers):
            print(json.dumps(rec), flush=True)
        sys.exit(0)
    if args.ops == "device":
        for rec in device_ops_rows(ctx, seeds, want, runs=args.runs, layers=layers):
            print(json.dumps(rec), flush=True)
        sys.exit(0)
    if args.compare:
        for rec in compare_compilers(ctx, seeds, want, runs=args.runs, layers=layers):
            print(json.dumps(rec), flush=True)
        sys.exit(0)
    if args.bench_record:  # bench.py's `streaming` record: the default chunk size only, one JSON line
        rec = streaming_record(ctx, prog, wit, wc, st, seeds, want, chunk_ops=1 << 18, layers=layers)
        rec["note"] += "; measured in a process of its own (tools/stream_bench.py --bench-record): inside bench.py's process -- 20+ GB of host arrays, the oracle's and torch's thread pools -- the host-side compile of the chunks runs ~1.5x slower (0.18 s)"
        print(json.dumps(rec))
        sys.exit(0)
    for chunk in (1 << 20, 1 << 18):
        print(json.dumps(streaming_record(ctx, prog, wit, wc, st, seeds, want, chunk_ops=chunk, layers=layers)))
    print(json.dumps(z64_record(ctx, seeds, n_mul=int(os.environ.get("Z64_MULS", "1000000")))))
