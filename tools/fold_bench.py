"""Constant folding (rv_ops_fold / rv_ops_fold_device) where it costs and where it pays.

    python tools/fold_bench.py [--runs 5] [--only ssa,sha,chain] [--small] [--leaves 64] [--windows [--window-ops 65536,1048576]]

One JSON line per case; every time is the median of --runs calls after one warm-up, with [min, max], in this one process:
  ssa    layered_gf2() (10^7 GF(2) gates in SSA form) with every 4th Input turned into a Const of the bit the witness had there
  sha    the SHA-256 Merkle tree of tools/link_bench.py with a second compression per node whose 512 message ports are bound to
         Consts in the netlist's head (the padding block of a two-block message): an all-constant message schedule per node
  chain  one known chain of 50 000 single ops behind 10^6 unknown ones (where the device path loses)
For each: rv_ops_fold, rv_ops_fold_device, rv_ops_prune_device on the same tensor, a hipMemcpyDtoD of the list, the work memory the
first device call of the process took beside its input and output (later calls find the arena's and torch's blocks: their figure
says nothing), the Muls folded, and (ssa, sha) Proof.new time and proof bytes before fold, after fold, and after fold + prune
(sha: pruned against the root's digest, the tree having no assertion).
--windows (rv_folder_*), on the same three lists in device memory, instead of the above: rv_ops_fold_device on the whole
list; for each window size one counting pass with the log kept (begin, a feed per window, end) -- its time, the tables' and the log's
bytes, the largest work memory of a feed, and whether a writing pass gives the whole-list call's bytes; then the replay pass over the
same windows into a second tensor, against a hipMemcpyDtoD of the list.
--small: the shapes of a smoke run (a quick layered_gf2, 4 leaves, a chain of 2 000 behind 10^4)."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402


def timed(fn, runs, between=None):
    """-> (last result, {median, min, max} in ms) of `runs` calls after one warm-up; between: called, untimed, before every call but
    the first"""
    fn()
    ts = []
    for _ in range(runs):
        if between is not None:
            between()
        t0 = time.perf_counter()
        r = fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    ts.sort()
    return r, {"ms": round(ts[len(ts) // 2], 3), "ms_min_max": [round(ts[0], 3), round(ts[-1], 3)]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--only", default="ssa,sha,chain")
    ap.add_argument("--small", action="store_true")
    ap.add_argument("--leaves", type=int, default=64, help="leaves of the Merkle tree, a power of two")
    ap.add_argument("--windows", action="store_true", help="measure the windowed folder instead")
    ap.add_argument("--window-ops", default=None, help="--windows: window sizes in ops (default 65536,1048576; --small: 1024,4096)")
    a = ap.parse_args()
    only = set(a.only.split(","))
    import torch

    import bristol_gen
    import circuits
    import reverie_amd as rv
    from link_bench import tree_tables
    from reverie_amd.link import Block, Netlist
    from reverie_amd.ops import GF2, OP_DTYPE, program

    import ctypes

    from reverie_amd import _lib

    ctx = rv.Context.default()
    L = _lib.lib()
    seeds = np.arange(4096, dtype=np.uint32).astype(np.uint8).reshape(256, 16)
    dev = lambda p: torch.from_numpy(np.ascontiguousarray(p).view(np.uint8).reshape(-1, 24).copy()).cuda()

    def fold_pair(prog, wc, rec):
        """host and device time of one list, and the yardsticks on the same tensor; -> the device result as a host array"""
        d_prog = dev(prog)
        (h_out, h_info), rec["host"] = timed(lambda: rv.fold_ops(prog, wc), a.runs)

        def on_device():
            r = rv.fold_ops(d_prog, wc, ctx=ctx)
            torch.cuda.synchronize()
            return r

        torch.cuda.synchronize()
        free_before = torch.cuda.mem_get_info()[0]
        first = on_device()
        rec["device_work_bytes_per_op"] = round((free_before - torch.cuda.mem_get_info()[0] - len(prog) * 24) / max(len(prog), 1), 1)
        del first
        (d_out, d_info), rec["device"] = timed(on_device, a.runs)
        _, rec["device_count_only"] = timed(lambda: rv.fold_ops(d_prog, wc, ctx=ctx, count_only=True), a.runs)

        def prune():
            r = rv.prune_ops(d_prog, wc, ctx=ctx)
            torch.cuda.synchronize()
            return r

        _, rec["prune_device_same_tensor"] = timed(prune, a.runs)
        room = torch.empty_like(d_prog)

        def dtod():
            room.copy_(d_prog)
            torch.cuda.synchronize()

        _, rec["memcpy_dtod"] = timed(dtod, a.runs)
        rec["device_over_host"] = round(rec["device"]["ms"] / rec["host"]["ms"], 3)
        rec["device_over_prune_device"] = round(rec["device"]["ms"] / rec["prune_device_same_tensor"]["ms"], 3)
        print("# %s: fold and yardsticks done" % rec["case"], file=sys.stderr, flush=True)
        rec["device_equals_host"] = bool(d_out.cpu().numpy().tobytes() == h_out.tobytes())
        rec["info"] = d_info
        rec["muls_folded"] = sum(d_info[k] for k in ("gf2_mul_to_const", "z64_mul_to_const", "gf2_mul_to_linear", "z64_mul_to_linear"))
        return h_out

    def windows_pair(prog, wc, rec):
        """--windows: the windowed pass at every window size against the whole-list call, and the replay pass against a copy"""
        from reverie_amd.fold import DeviceFolder

        d_prog = dev(prog)
        n = len(prog)

        def whole():
            r = rv.fold_ops(d_prog, wc, ctx=ctx)
            torch.cuda.synchronize()
            return r

        (want, w_info), rec["device_whole"] = timed(whole, a.runs)
        rec["n_rewritten"] = w_info["n_rewritten"]
        room = torch.empty_like(d_prog)

        def dtod():
            room.copy_(d_prog)
            torch.cuda.synchronize()

        _, rec["memcpy_dtod"] = timed(dtod, a.runs)
        sizes = [int(x) for x in (a.window_ops or ("1024,4096" if a.small else "65536,1048576")).split(",")]
        rec["windows"] = []
        for w in sizes:
            out = {"window_ops": w, "feeds": (n + w - 1) // w}
            df = DeviceFolder(wc, ctx=ctx, keep_log=True)
            try:
                def counting():
                    for at in range(0, n, w):
                        df.feed(d_prog[at:at + w], count_only=True)
                    info = df.end()
                    torch.cuda.synchronize()
                    return info

                # (the rewind between two passes clears every table entry: it is not part of a pass, and is not timed)
                info, out["counting_pass"] = timed(counting, a.runs, between=df.rewind)
                df.rewind()
                got = torch.cat([df.feed(d_prog[at:at + w]) for at in range(0, n, w)]) if n else d_prog
                info = df.end()
                out["equals_whole"] = bool(torch.equal(got, want)) and all(info[k] == w_info[k] for k in w_info if k not in ("device_rounds", "on_device"))
                out["device_rounds"], out["on_device"] = info["device_rounds"], info["on_device"]
                fi = df.get_info()
                out.update(state_bytes=fi["state_bytes"], log_bytes=fi["log_bytes"], log_records=fi["log_records"], peak_feed_bytes=fi["peak_feed_bytes"],
                           host_feeds=fi["host_feeds"])

                def replay():
                    for at in range(0, n, w):
                        L.rv_folder_replay(df.handle, ctypes.c_void_p(d_prog.data_ptr() + at * 24), min(w, n - at), 1, at, ctypes.c_void_p(room.data_ptr() + at * 24))
                    df.replay_end()
                    torch.cuda.synchronize()

                _, out["replay_pass"] = timed(replay, a.runs)
                out["replay_equals_whole"] = bool(torch.equal(room, want))
                out["counting_over_whole"] = round(out["counting_pass"]["ms"] / rec["device_whole"]["ms"], 3)
                out["replay_over_memcpy"] = round(out["replay_pass"]["ms"] / max(rec["memcpy_dtod"]["ms"], 1e-6), 3)
            finally:
                df.close()
            rec["windows"].append(out)
            print("# %s: windows of %d ops done" % (rec["case"], w), file=sys.stderr, flush=True)

    def proofs(prog, folded, wit, wc, rec, outs=()):
        pruned = rv.prune_ops(folded, wc, outputs_gf2=outs)[0]
        rec["ops_after_fold_and_prune"] = len(pruned)
        for name, ops in (("proof_original", prog), ("proof_folded", folded), ("proof_folded_pruned", pruned)):
            c = rv.Circuit(ops, wc, whole_prover=True)
            p, t = timed(lambda: rv.Proof.new(c, wit, [], seeds=seeds), a.runs)
            print("# %s: %s done" % (rec["case"], name), file=sys.stderr, flush=True)
            rec[name] = dict(t, proof_bytes=len(bytes(p)), verifies=bool(p.verify(c)))
            c.close()

    if "ssa" in only:
        prog, wit, wc, st = circuits.layered_gf2(n_in=64, width=256, layers=12) if a.small else circuits.layered_gf2()
        prog, wit = prog.copy(), np.asarray(wit, np.uint8)
        inputs = np.flatnonzero((prog["domain"] == 0) & (prog["opcode"] == 0))
        fixed = np.arange(len(inputs)) % 4 == 0
        prog["opcode"][inputs[fixed]], prog["imm"][inputs[fixed]] = 9, wit[fixed]  # the statement still holds
        rec = {"case": "ssa", "n_ops": len(prog), "inputs_made_const": int(fixed.sum()), "of": len(inputs), "runs": a.runs}
        if a.windows:
            windows_pair(prog, wc, rec)
        else:
            folded = fold_pair(prog, wc, rec)
            proofs(prog, folded, wit[~fixed], wc, rec)
        print(json.dumps(rec), flush=True)
    if "sha" in only:
        leaves = 4 if a.small else a.leaves
        block = Block.from_bristol(bristol_gen.sha256_block())
        pad = [1] + [0] * 501 + [(512 >> (9 - k)) & 1 for k in range(10)]  # the padding block of a 512-bit message
        head = program([GF2.Const(k, pad[k]) for k in range(512)])
        nodes = 2 * leaves - 1
        block_of, bindings = tree_tables(leaves, block.wire_counts[1], block.outputs, 512)
        padded = np.tile(np.arange(512, dtype=np.uint32), nodes)  # every node's second compression: its message is the head's
        nl = Netlist.from_arrays([block], np.concatenate([block_of, np.zeros(nodes, np.uint32)]), np.concatenate([bindings, padded]), head=head)
        prog, linfo = nl.link_host()
        wc = linfo["wire_counts"]
        wit = (np.arange(leaves * 512) * 7 % 5 < 2).astype(np.uint8)
        rec = {"case": "sha", "leaves": leaves, "instances": 2 * nodes, "n_ops": len(prog), "runs": a.runs}
        if a.windows:
            windows_pair(prog, wc, rec)
        else:
            folded = fold_pair(prog, wc, rec)
            root = 512 + (nodes - 1) * block.wire_counts[1] + np.asarray(block.outputs, np.int64)  # the tree has no assertion: its root digest is kept
            proofs(prog, folded, wit, wc, rec, root.tolist())
        print(json.dumps(rec), flush=True)
    if "chain" in only:
        live, depth = (10_000, 2_000) if a.small else (1_000_000, 50_000)
        ops = np.zeros(live + depth + 1, OP_DTYPE)
        body = ops[1:live]  # (ops[0] is Input(0))
        body["opcode"], body["dst"], body["a"], body["b"] = 2, np.arange(1, live), np.arange(0, live - 1), np.arange(0, live - 1)
        ops[live] = GF2.Const(live, 1)
        chain = ops[live + 1:]
        chain["opcode"], chain["dst"], chain["a"], chain["imm"] = 3, np.arange(live + 1, live + depth + 1), np.arange(live, live + depth), 1
        prog, wc = program(ops), (0, live + depth + 1)
        rec = {"case": "chain", "unknown": live, "known_chain": depth, "runs": a.runs}
        (windows_pair if a.windows else fold_pair)(prog, wc, rec)
        print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
