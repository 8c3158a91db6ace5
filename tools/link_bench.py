"""The linker (rv_link, rv_link_plan_*) on a SHA-256 Merkle tree: `bristol_gen.sha256_block` instanced once per node of a
tree with --leaves leaves (64: 127 instances, about the headline circuit's gate count), every inner node's 512 input ports bound to
its two children's digests, the leaves' ports left to the witness.

    python tools/link_bench.py [--leaves 64] [--runs 5] [--window-ops 4194304,262144] [--no-model] [--no-chain]

One JSON line with, each the median of --runs calls after one warm-up, with min and max: the numpy model of tests/link_ref.py
(--no-model leaves it out), the host rv_link, `plan.link_device()` into one buffer, the same list emitted in windows of --window-ops
records ("ms_per_call": the time above the whole-list call's, per emit), rv_link_plan_create on its own, a hipMemcpyDtoD of the
same number of bytes in the same process (the yardstick: the list cannot be written faster than it can be copied), and the upload of
the host-linked list from pageable memory (what the plan removes).  The chain (--no-chain leaves it out): the text of the one block
-> `Block.from_bristol(device=True)` -> plan -> `prove_streaming_pieces(plan.pieces(...))`, with and without compact_wires, with the
streams' wire store in bytes; the two proofs are checked to be the same bytes."""
import argparse
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402

from bincode_bench import timed  # noqa: E402


def tree_tables(leaves: int, wires: int, outputs, base: int):
    """-> (block_of, bindings) of a binary tree over one block of 512 ports: instances 0 .. leaves - 1 are the leaves, then level by
    level up to the root; an inner node's ports are its left child's outputs, then its right child's"""
    from reverie_amd.link import WITNESS

    outs = np.asarray(outputs, dtype=np.uint64)
    bind = [np.full(leaves * 512, WITNESS, dtype=np.uint32)]
    first, width = 0, leaves
    while width > 1:
        kids = first + np.arange(width, dtype=np.uint64)  # this level's nodes, two per parent
        bind.append((base + kids[:, None] * np.uint64(wires) + outs[None, :]).astype(np.uint32).reshape(-1))
        first, width = first + width, width // 2
    return np.zeros(2 * leaves - 1, np.uint32), np.concatenate(bind)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--leaves", type=int, default=64, help="a power of two")
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--window-ops", default="4194304,262144", help="comma-separated records per emit")
    ap.add_argument("--no-model", action="store_true", help="leave out the numpy model")
    ap.add_argument("--no-chain", action="store_true")
    a = ap.parse_args()
    assert a.leaves >= 2 and a.leaves & (a.leaves - 1) == 0
    window_ops = [int(x) for x in a.window_ops.split(",") if x]
    import torch

    import bristol_gen
    import link_ref
    import reverie_amd as rv
    from reverie_amd import _lib, stream
    from reverie_amd.link import Block, Netlist
    from reverie_amd.ops import OP_DTYPE

    REC = OP_DTYPE.itemsize
    ctx = rv.Context.default()
    text = bristol_gen.sha256_block()
    block = Block.from_bristol(text)
    assert block.n_ports == 512 and len(block.outputs) == 256
    block_of, bindings = tree_tables(a.leaves, block.wire_counts[1], block.outputs, 0)
    nl = Netlist.from_arrays([block], block_of, bindings)
    host, info = nl.link_host()
    rec = {"leaves": a.leaves, "instances": info["n_instances"], "block_ops": len(block.ops), "n_ops": info["n_ops"], "bytes": info["n_ops"] * REC,
           "gf2_wires": info["gf2_wires"], "n_input_gf2": info["n_input_gf2"], "runs": a.runs}

    if not a.no_model:
        spec = link_ref.Spec([(block.ops, block.wire_counts)], block_of, bindings)
        (code, model, minfo), t = timed(lambda: link_ref.link(spec), a.runs)
        rec.update({"numpy_model": t, "model_equals_host": bool(code == 0 and model.tobytes() == host.tobytes() and minfo == info)})
        del model
    _, rec["rv_link"] = timed(nl.link_host, a.runs)

    plan, rec["plan_create"] = timed(lambda: nl.plan(ctx), a.runs)
    out = torch.empty((info["n_ops"], REC), dtype=torch.uint8, device=f"cuda:{ctx.device}")

    def whole():
        for first in range(0, info["n_ops"], (1 << 28) - 256):
            n = min((1 << 28) - 256, info["n_ops"] - first)
            plan.emit(first, n, out[first:first + n])

    _, rec["link_device"] = timed(whole, a.runs)
    rec["device_equals_host"] = bool(out.cpu().numpy().tobytes() == host.tobytes())
    rec["windows"] = {}
    for per in window_ops:
        def windows():
            for first in range(0, info["n_ops"], per):
                n = min(per, info["n_ops"] - first)
                plan.emit(first, n, out[first:first + n])

        out.zero_()
        _, t = timed(windows, a.runs)
        calls = -(-info["n_ops"] // per)
        t.update({"calls": calls, "ms_per_call": (t["ms"] - rec["link_device"]["ms"]) / calls, "equals_host": bool(out.cpu().numpy().tobytes() == host.tobytes())})
        rec["windows"][str(per)] = t

    # the yardstick: a device-to-device copy of as many bytes, through the runtime this process already runs
    src = torch.empty_like(out)
    hip = None
    for name in ("libamdhip64.so", "libamdhip64.so.6", "libamdhip64.so.7"):
        try:
            hip = C.CDLL(name)
            break
        except OSError:
            pass
    if hip is not None and hasattr(hip, "hipMemcpyDtoD"):
        hip.hipMemcpyDtoD.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t]

        def dtod():
            assert hip.hipMemcpyDtoD(out.data_ptr(), src.data_ptr(), out.numel()) == 0
            assert hip.hipDeviceSynchronize() == 0

        rec["copy_call"] = "hipMemcpyDtoD"
    else:
        def dtod():
            out.copy_(src)
            torch.cuda.synchronize()

        rec["copy_call"] = "torch copy_"
    _, rec["device_copy"] = timed(dtod, a.runs)
    rec["link_over_copy"] = rec["link_device"]["ms"] / rec["device_copy"]["ms"]

    def upload():
        t = torch.from_numpy(host.view(np.uint8)).to(f"cuda:{ctx.device}")
        torch.cuda.synchronize()
        return t

    _, rec["upload_host_list"] = timed(upload, a.runs)
    plan.close()
    del out, src

    if not a.no_chain:
        rng = np.random.default_rng(7)
        wit = rng.integers(0, 2, info["n_input_gf2"]).astype(np.uint8)
        seeds = rng.integers(0, 256, (256, 16)).astype(np.uint8)
        proofs = {}

        def chain(compact):
            def run():
                blk = Block.from_bristol(text, ctx=ctx, device=True)
                with Netlist.from_arrays([blk], block_of, bindings).plan(ctx) as p:
                    proof, sinfo = stream.prove_streaming_pieces(p.pieces(window_ops[0]), wit, [], p.info["wire_counts"], seeds=seeds, ctx=ctx,
                                                                 device_compile=True, compact_wires=compact)
                proofs[compact] = bytes(proof)
                return sinfo

            sinfo, t = timed(run, a.runs)
            t["wire_store_bytes"] = int(sinfo["wire_store_bytes"])
            return t

        rec["text_to_streamed_proof"] = chain(False)
        rec["text_to_streamed_proof_compact_wires"] = chain(True)
        rec["chain_proofs_agree"] = proofs[False] == proofs[True]
        rec["proof_bytes"] = len(proofs[False])
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
