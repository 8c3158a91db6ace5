"""The Bristol parser on the GPU (rv_bristol_parse_device) beside the host parser, on the headline circuit written as text.

    python tools/bristol_bench.py [--text host|device] [--gates N] [--runs 5] [--window-mb 64,4] [--no-chain]

The SSA form of the benchmark circuit (layered_gf2(recycle=False); --gates N: about N gates of the same shape) is written as Bristol
Fashion text by bristol.dumps, its assertion tail as expected outputs.  Both parsers are checked once to give the same records (and
those to be the generator's).  One JSON line with, each the median of --runs calls after one warm-up, with min and max: rv_bristol_parse;
rv_bristol_parse_device from host text; the same from text in GPU memory (the difference is the upload); and the chain from text to
proof -- parse_device -> rv_circuit_compile_device -> rv_prove, with the text where --text says -- beside its all-host counterpart
(rv_bristol_parse -> rv_circuit_compile -> rv_prove; --no-chain leaves both chains out).  The baseline and the device path run in one
process, on the same text.  --window-mb 64,4: the same text read through rv_bristol_reader_* in windows of that many MiB,
from host bytes and from the GPU tensor, every feed writing into one buffer of len / 6 + 1 + inputs + pairs records; the pieces are
checked once to be the whole-text call's records."""
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--text", default="host", choices=["host", "device"])
    ap.add_argument("--gates", type=int, default=0, help="about this many gates (0: the headline circuit, 65536 x 153)")
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--window-mb", default="", help="comma-separated window sizes in MiB for the windowed reader (e.g. 64,4)")
    ap.add_argument("--no-chain", action="store_true", help="leave out the two text-to-proof chains")
    a = ap.parse_args()
    import torch

    import circuits
    import reverie_amd as rv
    from reverie_amd import _lib, bristol
    from reverie_amd.ops import OP_DTYPE

    if a.gates:
        width = 65536 if a.gates >= (1 << 20) else 1024
        prog, wit, wc, st = circuits.layered_gf2(width=width, layers=max(1, a.gates // width))
    else:
        prog, wit, wc, st = circuits.layered_gf2()
    k = int(np.count_nonzero(prog["opcode"] == 8))  # the assertion tail: AddConst + AssertZero per output
    exp = prog["imm"][-2 * k::2].astype(np.uint8)
    t0 = time.perf_counter()
    text = bristol.dumps(prog[:-2 * k], k)
    t_dumps = time.perf_counter() - t0
    ctx = rv.Context.default()
    seeds = np.arange(4096, dtype=np.uint32).astype(np.uint8).reshape(256, 16)
    h_text = np.frombuffer(text, np.uint8)
    d_text = torch.from_numpy(h_text.copy()).cuda()
    L = _lib.lib()

    def host():
        ops, n, bi = C.c_void_p(), C.c_size_t(), _lib.BristolInfo()
        _lib.check(L.rv_bristol_parse(C.c_void_p(h_text.ctypes.data), C.c_size_t(h_text.size), 0, C.c_void_p(exp.ctypes.data), C.c_size_t(k),
                                      C.byref(ops), C.byref(n), C.byref(bi)))
        out = np.frombuffer(C.string_at(ops, n.value * OP_DTYPE.itemsize), dtype=OP_DTYPE)
        L.rv_free(ops)
        return out, int(bi.gf2_wires)

    d_ops = torch.empty((len(prog), OP_DTYPE.itemsize), dtype=torch.uint8, device="cuda")

    def device(src, on_device):  # (the records' room is there: the C call alone)
        n, bi = C.c_size_t(), _lib.BristolInfo()
        _lib.check(L.rv_bristol_parse_device(ctx.handle, C.c_void_p(src), C.c_size_t(h_text.size), on_device, 0, C.c_void_p(exp.ctypes.data), C.c_size_t(k),
                                             C.c_void_p(d_ops.data_ptr()), C.c_size_t(len(prog)), C.byref(n), C.byref(bi)))
        return int(n.value), int(bi.gf2_wires)

    (h_ops, h_wires), t_host = timed(host, a.runs)
    (n_dev, d_wires), t_dev_host = timed(lambda: device(h_text.ctypes.data, 0), a.runs)
    d_ops.zero_()
    (_, _), t_dev_dev = timed(lambda: device(d_text.data_ptr(), 1), a.runs)
    same = n_dev == len(h_ops) and d_wires == h_wires and d_ops.cpu().numpy().tobytes() == h_ops.tobytes()
    rec = {"gates": st["gates"], "n_ops": len(prog), "text_bytes": len(text), "dumps_s": t_dumps, "runs": a.runs,
           "parsers_agree": bool(same), "parse_equals_generator": h_ops.tobytes() == prog.tobytes(),
           "host_parse": t_host, "device_parse_host_text": t_dev_host, "device_parse_device_text": t_dev_dev}

    def windows(src, on_device, window, keep=None):
        """the text in windows of `window` bytes through the C calls; keep: a tensor that receives all records (the check)"""
        r, piece, total = C.c_void_p(), _lib.BristolPiece(), 0
        _lib.check(L.rv_bristol_reader_begin(ctx.handle, C.c_uint64(h_text.size), 0, C.c_void_p(exp.ctypes.data), C.c_size_t(k), C.byref(r)))
        try:
            for at in range(0, h_text.size, window):
                n = min(window, h_text.size - at)
                _lib.check(L.rv_bristol_reader_feed(r, C.c_void_p(src + at), C.c_size_t(n), on_device, C.c_void_p(w_ops.data_ptr()), C.c_size_t(w_ops.shape[0]),
                                                    C.byref(piece)))
                if keep is not None:
                    keep[piece.first_op:piece.first_op + piece.n_ops] = w_ops[:piece.n_ops]
                total += piece.n_ops
            _lib.check(L.rv_bristol_reader_finish(r, None))
        finally:
            L.rv_bristol_reader_destroy(r)
        return total

    for mb in [int(x) for x in a.window_mb.split(",") if x]:
        window = mb << 20
        n_in = int(np.count_nonzero(prog["opcode"] == 0))
        w_ops = torch.empty((2 * window // 6 + 2 + n_in + 2 * k, OP_DTYPE.itemsize), dtype=torch.uint8, device="cuda")
        keep = torch.zeros_like(d_ops)
        ok = windows(d_text.data_ptr(), 1, window, keep) == len(prog) and torch.equal(keep, d_ops)
        del keep
        _, t_wh = timed(lambda: windows(h_text.ctypes.data, 0, window), a.runs)
        _, t_wd = timed(lambda: windows(d_text.data_ptr(), 1, window), a.runs)
        rec["windows_%d_mib" % mb] = {"feeds": -(-h_text.size // window), "same_records": bool(ok), "host_text": t_wh, "device_text": t_wd}
        del w_ops
    if a.no_chain:
        print(json.dumps(rec))
        return

    def chain_host():
        ops, info = bristol.parse(text, expected_outputs=exp)
        return bytes(rv.Proof.new(rv.Circuit(ops, info["wire_counts"]), wit, [], seeds=seeds))

    def chain_device():
        ops, info = bristol.parse_device(d_text if a.text == "device" else h_text, expected_outputs=exp, device=ctx)
        return bytes(rv.Proof.new(rv.Circuit.from_device_ops(ops, info["wire_counts"], ctx), wit, [], seeds=seeds))

    p_host, t_chain_host = timed(chain_host, a.runs)
    p_dev, t_chain_dev = timed(chain_device, a.runs)
    rec.update({"chain_text": a.text, "chain_host": t_chain_host, "chain_device": t_chain_dev, "same_proof": p_host == p_dev})
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
