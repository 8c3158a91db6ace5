"""Pruning (rv_ops_prune / rv_ops_prune_device) where it costs and where it pays.

    python tools/prune_bench.py [--runs 5] [--only as-is,sixteenth,aes,chain] [--small] [--window-ops N[,N]]

One JSON line per case; every time is the median of --runs calls after one warm-up, with [min, max], in this one process:
  as-is      layered_gf2() (10^7 GF(2) gates in SSA form) as it is -- little is dead: the device call against the host sweep and
             against rv_ops_compact_wires_device on the same tensor (the same classify, sort and resolve), the counting call (all
             but the emit), the work memory the first device call of the process took beside its input and output (later calls
             find the arena's and torch's blocks: their figure says nothing)
  sixteenth  the same list with only every 16th assertion pair of its tail kept, so that a dead cone opens backwards: dropped ops
             by class, device_rounds, host and device time, Proof.new time and proof bytes before and after
  aes        1 024 AES-128 instances through reverie_amd.link, the tail asserting one output byte of each: the same figures, and
             text -> Block.from_bristol(device=True) -> plan -> link_device -> prove_streaming with and without prune=True
  chain      one dead chain of 50 000 single ops behind a live list of 10^6: device against host (where the device path loses), and
             the device call under RV_PRUNE_MAX_ROUNDS=1024 (the fall-back)
--window-ops N[,N]: on as-is and aes, the same tensor through rv_pruner_* in windows of N ops -- the scan pass, the
mark pass (last window first) and one emit pass timed apart, against the whole-list device call of the same process; the cost per
feed above the whole call, state_bytes and peak_feed_bytes; and on aes the chain the windows are for: plan.pieces(N) -> the streamed
proof with compact_wires=True, with and without prune=True, the list never whole.
--small: the shapes of a smoke run (a quick layered_gf2, 16 AES instances, a chain of 2 000 behind 10^4)."""
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
    return r, {"ms": round(ts[len(ts) // 2], 3), "ms_min_max": [round(ts[0], 3), round(ts[-1], 3)]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--only", default="as-is,sixteenth,aes,chain")
    ap.add_argument("--small", action="store_true")
    ap.add_argument("--window-ops", default="", help="window sizes for the windowed pruner, comma separated")
    a = ap.parse_args()
    only = set(a.only.split(","))
    window_ops = [int(x) for x in a.window_ops.split(",") if x]
    import torch

    import bristol_gen
    import circuits
    import reverie_amd as rv
    from reverie_amd.ops import GF2, OP_DTYPE, program

    ctx = rv.Context.default()
    seeds = np.arange(4096, dtype=np.uint32).astype(np.uint8).reshape(256, 16)
    dev = lambda p: torch.from_numpy(np.ascontiguousarray(p).view(np.uint8).reshape(-1, 24).copy()).cuda()

    def prune_pair(prog, wc, rec):
        """host and device time of one list; -> (the device result, its info)"""
        d_prog = dev(prog)
        (h_out, h_info, _), rec["host"] = timed(lambda: rv.prune_ops(prog, wc), a.runs)

        def on_device():
            r = rv.prune_ops(d_prog, wc, ctx=ctx)
            torch.cuda.synchronize()
            return r

        torch.cuda.synchronize()
        free_before = torch.cuda.mem_get_info()[0]
        first = on_device()
        rec["device_work_bytes_per_op"] = round((free_before - torch.cuda.mem_get_info()[0] - len(prog) * 28) / max(len(prog), 1), 1)
        del first
        (d_out, d_info, d_old), rec["device"] = timed(on_device, a.runs)
        # the counting call runs everything but the flags' sum and the emit: the difference is what writing the list costs
        _, rec["device_count_only"] = timed(lambda: rv.prune_ops(d_prog, wc, ctx=ctx, count_only=True), a.runs)
        rec["device_equals_host"] = bool(d_out.cpu().numpy().tobytes() == h_out.tobytes())
        rec["info"] = d_info
        return d_prog, d_out, d_info

    def windowed(d_prog, wc, rec, want):
        """the three passes of rv_pruner_* over the tensor in windows of each --window-ops size, timed apart"""
        from reverie_amd.prune import DevicePruner

        n = len(d_prog)
        for w in window_ops:
            firsts = list(range(0, n, w))
            passes = {"scan": [], "mark": [], "emit": []}
            for run in range(a.runs + 1):  # (the first is the warm-up)
                with DevicePruner(wc, ctx=ctx) as dp:
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    for f in firsts:
                        dp.scan(d_prog[f:f + w])
                    dp.scan_end()
                    t1 = time.perf_counter()
                    for f in reversed(firsts):
                        dp.mark(d_prog[f:f + w])
                    info = dp.mark_end()
                    t2 = time.perf_counter()
                    outs = [dp.feed(d_prog[f:f + w])[0] for f in firsts]
                    torch.cuda.synchronize()
                    t3 = time.perf_counter()
                    pinfo = dp.get_info()
                    if run == 0:
                        same = bool(torch.cat(outs).cpu().numpy().tobytes() == want.cpu().numpy().tobytes())
                    del outs
                if run:
                    for k, t in zip(("scan", "mark", "emit"), (t1 - t0, t2 - t1, t3 - t2)):
                        passes[k].append(t * 1e3)
            r = {"feeds": len(firsts), "equals_whole_call": same, "device_rounds": info["device_rounds"], "on_device": info["on_device"],
                 "state_bytes": pinfo["state_bytes"], "peak_feed_bytes": pinfo["peak_feed_bytes"], "host_feeds": pinfo["host_feeds"]}
            total = 0.0
            for k, ts in passes.items():
                ts.sort()
                r[k] = {"ms": round(ts[len(ts) // 2], 3), "ms_min_max": [round(ts[0], 3), round(ts[-1], 3)]}
                total += ts[len(ts) // 2]
            r["three_passes_ms"] = round(total, 3)
            r["per_feed_ms_above_whole_call"] = round((total - rec["device"]["ms"]) / (3 * len(firsts)), 4)
            rec["windows_%d" % w] = r

    def proofs(prog, wit, wc, pruned, rec):
        for name, ops in (("proof_original", prog), ("proof_pruned", pruned)):
            c = rv.Circuit(ops, wc, whole_prover=True)
            p, t = timed(lambda: rv.Proof.new(c, wit, [], seeds=seeds), a.runs)
            rec[name] = dict(t, proof_bytes=len(bytes(p)), verifies=bool(p.verify(c)))
            c.close()

    gen = (lambda: circuits.layered_gf2(n_in=64, width=256, layers=12)) if a.small else circuits.layered_gf2
    if only & {"as-is", "sixteenth"}:
        prog, wit, wc, st = gen()
    if "as-is" in only:
        rec = {"case": "as-is", "n_ops": len(prog), "runs": a.runs}
        d_prog, d_whole, _ = prune_pair(prog, wc, rec)
        windowed(d_prog, wc, rec, d_whole)

        def compact():
            r = rv.compact_wires(d_prog, wc, ctx)
            torch.cuda.synchronize()
            return r

        _, rec["compact_wires_device"] = timed(compact, a.runs)
        rec["prune_over_compact"] = round(rec["device"]["ms"] / rec["compact_wires_device"]["ms"], 3)
        print(json.dumps(rec), flush=True)
    if "sixteenth" in only:
        k = int(np.count_nonzero(prog["opcode"] == 8))  # the tail: AddConst + AssertZero per folded wire
        tail = prog[-2 * k:].reshape(k, 2)
        cut = np.concatenate([prog[:-2 * k], tail[::16].reshape(-1)])
        rec = {"case": "sixteenth", "n_ops": len(cut), "assertions_kept": int(len(tail[::16])), "of": k, "runs": a.runs}
        _, d_out, info = prune_pair(cut, wc, rec)
        proofs(cut, wit, wc, d_out.cpu().numpy().reshape(-1).view(OP_DTYPE), rec)
        print(json.dumps(rec), flush=True)
    if "aes" in only:
        n_inst = 16 if a.small else 1024
        text = bristol_gen.aes128() if hasattr(bristol_gen, "aes128") else None
        if text is None:
            print(json.dumps({"case": "aes", "skipped": "tests/bristol_gen.py has no aes128()"}), flush=True)
        else:
            block = rv.Block.from_bristol(text)
            nl = rv.Netlist([block])
            tail = []
            insts = [nl.add(0, [rv.link.WITNESS] * block.n_ports) for _ in range(n_inst)]
            scratch = nl.gf2_base + n_inst * block.wire_counts[1]
            wit = np.zeros(n_inst * block.n_ports, np.uint8)
            values = bristol_gen.evaluate(np.concatenate([block.ops]), [0] * block.n_ports)
            for inst in insts:
                for o_local, o in list(zip(block.outputs, inst.outputs))[:8]:
                    tail += [GF2.AddConst(scratch, o, values[o_local]), GF2.AssertZero(scratch)]
            nl.set_tail(tail)
            prog, linfo = nl.link_host()
            wc = linfo["wire_counts"]
            rec = {"case": "aes", "instances": n_inst, "n_ops": len(prog), "runs": a.runs}
            d_prog, d_out, info = prune_pair(prog, wc, rec)
            windowed(d_prog, wc, rec, d_out)
            proofs(prog, wit, wc, d_out.cpu().numpy().reshape(-1).view(OP_DTYPE), rec)
            del d_prog

            def never_whole(w, prune):
                b = rv.Block.from_bristol(text, device=True)
                nl2 = rv.Netlist([b])
                for _ in range(n_inst):
                    nl2.add(0, [rv.link.WITNESS] * b.n_ports)
                nl2.set_tail(tail)
                with nl2.plan(ctx) as plan:
                    p, sinfo = rv.stream.prove_streaming_pieces(plan.pieces(w), wit, [], wc, seeds=seeds, ctx=ctx, device_compile=True, prune=prune,
                                                                compact_wires=True)
                return len(bytes(p))

            for w in window_ops:
                for prune in (False, True):
                    n_bytes, t = timed(lambda: never_whole(w, prune), a.runs)
                    rec["pieces_%d_to_streamed_proof%s" % (w, "_pruned" if prune else "")] = dict(t, proof_bytes=n_bytes)

            def chain(prune):
                b = rv.Block.from_bristol(text, device=True)
                nl2 = rv.Netlist([b])
                for _ in range(n_inst):
                    nl2.add(0, [rv.link.WITNESS] * b.n_ports)
                nl2.set_tail(tail)
                with nl2.plan(ctx) as plan:
                    ops = plan.link_device()
                p, sinfo = rv.prove_streaming(ops, wit, [], wc, seeds=seeds, ctx=ctx, device_compile=True, prune=prune, compact_wires=True)
                return len(bytes(p))

            for prune in (False, True):
                n_bytes, t = timed(lambda: chain(prune), a.runs)
                rec["text_to_streamed_proof" + ("_pruned" if prune else "")] = dict(t, proof_bytes=n_bytes)
            print(json.dumps(rec), flush=True)
    if "chain" in only:
        live, depth = (10_000, 2_000) if a.small else (1_000_000, 50_000)
        ops = np.zeros(live + depth + 1, OP_DTYPE)
        ops["opcode"][0] = 0  # Input(0)
        body = ops[1:live]
        body["opcode"], body["dst"], body["a"], body["b"] = 2, np.arange(1, live), np.arange(0, live - 1), np.arange(0, live - 1)
        ops[live] = GF2.AssertZero(live - 1)
        dead = ops[live + 1:]
        dead["opcode"], dead["dst"], dead["a"], dead["imm"] = 3, np.arange(live, live + depth), np.arange(live - 1, live + depth - 1), 1
        prog, wc = program(ops), (0, live + depth)
        rec = {"case": "chain", "live": live, "dead_chain": depth, "runs": a.runs}
        prune_pair(prog, wc, rec)
        os.environ["RV_PRUNE_MAX_ROUNDS"] = "1024"
        d_prog = dev(prog)
        (_, finfo, _), rec["device_with_fallback_at_1024"] = timed(lambda: rv.prune_ops(d_prog, wc, ctx=ctx), a.runs)
        del os.environ["RV_PRUNE_MAX_ROUNDS"]
        rec["fallback_on_device"] = finfo["on_device"]
        print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
