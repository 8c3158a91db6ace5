"""Wire compaction (rv_ops_compact_wires / rv_ops_compact_wires_device) on the SSA forms of the benchmark circuits.

    python tools/compact_bench.py [--ops host|device] [--runs 5] [--no-ssa-stream] [--window-ops N[,N]] [--only-windows] [--bristol-window-mb N] [4|5|small]

config 4 = layered_gf2() (10^7 GF(2) gates), config 5 = layered_z64() (10^6 Z64 multiplications), small = a quick layered_gf2.  One JSON
line with: the wire counts before and after; the host sweep's time and the device path's time (each the median of --runs calls after
one warm-up, with min and max); rv_stream_info.wire_store_bytes of a streamed proof of the SSA list and of the compacted list; the
streamed proof's time on the compacted list beside the generator's own recycle=True numbering, measured in this process; and whether
the three proofs are the same bytes.  --ops device: the streamed proofs are fed from a GPU tensor (the compacted list is the device
path's output, which never visits the host); the default feeds host memory.  --no-ssa-stream: skip the streamed proof of the SSA list
(config 5's needs 18 KiB of wire store per gate).  --window-ops N[,N]: the windowed compactor (rv_compactor_*) on the
same list in feeds of N ops -- scan pass, rewrite pass and both together (medians as above), the per-feed cost that follows, its
state_bytes and peak_feed_bytes, whether the records are the whole-list call's; --ops device feeds slices of the GPU tensor, the
default uploads host slices.  --only-windows (a switch; the config stays the positional argument): stop after these (no streamed
proofs).  whole_list_call_work_bytes: the device memory the first whole-list device call took beside its input and output (the free
device memory before and after it: the arena keeps its blocks).  --bristol-window-mb N (configs 4 and small): file -> streamed proof --
the list as Bristol text (bristol.dumps, the assertion tail as expected outputs) through bristol.iter_device in windows of N MiB
and prove_streaming_pieces, as it is and with compact_wires=True: time, wire_store_bytes and whether the proofs are the same bytes;
nothing else is run then."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402


def timed(fn, runs):
    """-> (last result, {median, min, max} in ms) of `runs` calls after one warm-up"""
    fn()
    ts = []
    for _ in range(runs):
        t0 = time.perf_counter()
        r = fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    ts.sort()
    return r, {"ms": ts[len(ts) // 2], "ms_min_max": [ts[0], ts[-1]]}


def bristol_chain(a, rv, prog, wit, wc, seeds):
    from reverie_amd import bristol, stream

    if a.config == "5":
        raise SystemExit("--bristol-window-mb takes a GF(2) config (4 or small)")
    k = int(np.count_nonzero(prog["opcode"] == 8))  # the assertion tail: AddConst + AssertZero per output
    exp = prog["imm"][-2 * k::2].astype(np.uint8)
    text = np.frombuffer(bristol.dumps(prog[:-2 * k], k), np.uint8)
    window = a.bristol_window_mb << 20
    rec = {"config": a.config, "n_ops": len(prog), "text_bytes": int(text.size), "window_mb": a.bristol_window_mb, "runs": a.runs}
    proofs = {}
    for name, kw in (("compacted_in_windows", {"compact_wires": True}), ("as_it_is", {})):
        (p, info), t = timed(lambda: stream.prove_streaming_pieces(lambda: bristol.iter_device(text, window, exp), wit, [], wc, seeds=seeds, **kw), a.runs)
        proofs[name] = bytes(p)
        rec[name] = dict(t, wire_store_bytes=info["wire_store_bytes"], chunks=info["chunks"], compact=info.get("compact"))
    rec["same_proof"] = proofs["compacted_in_windows"] == proofs["as_it_is"]
    print(json.dumps(rec))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("config", nargs="?", default="4", choices=["4", "5", "small"])
    ap.add_argument("--ops", default="host", choices=["host", "device"])
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--no-ssa-stream", action="store_true")
    ap.add_argument("--window-ops", default="", help="feed sizes of the windowed compactor, comma separated")
    ap.add_argument("--only-windows", action="store_true")
    ap.add_argument("--bristol-window-mb", type=int, default=0)
    a = ap.parse_args()
    import torch

    import circuits
    import reverie_amd as rv

    gen = {"4": circuits.layered_gf2, "5": circuits.layered_z64, "small": lambda recycle=False: circuits.layered_gf2(n_in=64, width=256, layers=12, recycle=recycle)}[a.config]
    prog, wit, wc, st = gen()
    rprog, rwit, rwc, _ = gen(recycle=True)
    w2, w64 = (wit, []) if a.config != "5" else ([], wit)
    ctx = rv.Context.default()
    seeds = np.arange(4096, dtype=np.uint32).astype(np.uint8).reshape(256, 16)
    if a.bristol_window_mb:
        return bristol_chain(a, rv, prog, wit, wc, seeds)
    d_prog = torch.from_numpy(prog.view(np.uint8).reshape(-1, 24).copy()).cuda()

    (h_new, counts, info), t_host = timed(lambda: rv.compact_wires(prog, wc), a.runs)

    def on_device():
        r = rv.compact_wires(d_prog, wc, ctx)
        torch.cuda.synchronize()
        return r

    torch.cuda.synchronize()
    free_before = torch.cuda.mem_get_info()[0]
    first = on_device()
    work_bytes = free_before - torch.cuda.mem_get_info()[0] - first[0].numel() * first[0].element_size()
    del first
    (d_new, d_counts, d_info), t_dev = timed(on_device, a.runs)
    same = d_counts == counts and d_info == info and d_new.cpu().numpy().tobytes() == h_new.tobytes()
    rec = {"config": a.config, "n_ops": len(prog), "stats": st, "ops": a.ops, "wire_counts_ssa": list(wc), "wire_counts_compacted": list(counts),
           "wire_counts_recycled_by_hand": list(rwc), "info": info, "sweep": t_host, "device": t_dev, "device_equals_sweep": bool(same),
           "whole_list_call_work_bytes": int(work_bytes)}

    from reverie_amd.compact import DeviceCompactor

    def windowed(n_window):
        """-> ({scan, rewrite, total} timings, compactor info, same records) of the list in feeds of n_window ops"""
        src = d_prog if a.ops == "device" else prog
        cuts = list(range(0, len(prog), n_window))
        out = torch.empty_like(d_prog)
        laps = {"scan": [], "rewrite": []}
        for _ in range(a.runs + 1):
            with DeviceCompactor(wc, ctx) as dc:
                t0 = time.perf_counter()
                again = True
                while again:
                    for at in cuts:
                        dc.scan(src[at:at + n_window])
                    again = dc.scan_end()
                t1 = time.perf_counter()
                for at in cuts:
                    dc.feed(src[at:at + n_window], out=out[at:at + n_window])
                torch.cuda.synchronize()
                t2 = time.perf_counter()
                cinfo, w_info, w_counts = dc.get_info(), dc.info, dc.wire_counts
            laps["scan"].append((t1 - t0) * 1e3), laps["rewrite"].append((t2 - t1) * 1e3)
        t = {}
        for k, v in dict(laps, total=[x + y for x, y in zip(laps["scan"], laps["rewrite"])]).items():
            v = sorted(v[1:])  # (the first pass is the warm-up)
            t[k] = {"ms": v[len(v) // 2], "ms_min_max": [v[0], v[-1]]}
        t["ms_per_feed"] = t["total"]["ms"] / max(1, len(cuts) * (cinfo["scans"] + 1))
        same = w_counts == counts and w_info == info and out.cpu().numpy().tobytes() == h_new.tobytes()
        return dict(t, feeds=len(cuts), compactor=cinfo, equals_sweep=bool(same))

    if a.window_ops:
        rec["windows"] = {n: windowed(int(n)) for n in a.window_ops.split(",")}
    if a.only_windows:
        print(json.dumps(rec))
        return

    def stream(ops, counts_):
        return rv.prove_streaming(ops, w2, w64, counts_, seeds=seeds, ctx=ctx)

    on = (lambda p: torch.from_numpy(p.view(np.uint8).reshape(-1, 24).copy()).cuda()) if a.ops == "device" else (lambda p: p)
    (p_new, i_new), t_new = timed(lambda: stream(d_new if a.ops == "device" else h_new, counts), a.runs)
    r_ops = on(rprog)
    (p_rec, i_rec), t_rec = timed(lambda: stream(r_ops, rwc), a.runs)
    rec["stream_compacted"] = dict(t_new, wire_store_bytes=i_new["wire_store_bytes"], chunks=i_new["chunks"])
    rec["stream_recycled_by_hand"] = dict(t_rec, wire_store_bytes=i_rec["wire_store_bytes"], chunks=i_rec["chunks"])
    rec["same_proof_compacted_vs_recycled"] = bytes(p_new) == bytes(p_rec)
    if not a.no_ssa_stream:
        try:
            t0 = time.perf_counter()
            p_ssa, i_ssa = stream(d_prog if a.ops == "device" else prog, wc)
            rec["stream_ssa"] = {"ms_one_call": (time.perf_counter() - t0) * 1e3, "wire_store_bytes": i_ssa["wire_store_bytes"], "chunks": i_ssa["chunks"]}
            rec["same_proof_compacted_vs_ssa"] = bytes(p_new) == bytes(p_ssa)
        except rv.ReverieError as e:
            rec["stream_ssa"] = {"error": str(e)}
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
