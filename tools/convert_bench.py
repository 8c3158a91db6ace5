"""The writers on the GPU (rv_bristol_write_device, rv_bristol_writer_*, rv_program_writer_*) beside the host writers, on
the SSA form of the headline circuit, and `--operation convert` end to end.

    python tools/convert_bench.py [--gates N] [--runs 5] [--window-ops 4194304,262144] [--window-mb 64] [--no-dumps] [--no-chain]
                                  [--parent-lib PATH]

The SSA 10^7-gate list (layered_gf2(); --gates N: about N gates of the same shape) without its assertion tail is the Bristol writers'
input, the whole list the program-file writers'.  One JSON line with, each the median of --runs calls after one warm-up, with min and
max: rv_bristol_write_device beside the host rv_bristol_write and (one call; --no-dumps leaves it out) numpy's bristol.dumps;
rv_program_to_bincode_device; both windowed writers at --window-ops records per feed, from the op list in GPU memory into one buffer
("ms_per_feed": the time above the whole-list call's, per feed).  Every writer is checked once to give the host writer's bytes.
--parent-lib PATH: a build of another commit's library; its rv_program_to_bincode_device is called in turn with this tree's, each on
a fresh context of its own, this tree first and then the parent first ("program_write_alt": {"this", "parent", "parent_first"}).
The chain (--no-chain leaves it out): the list as Bristol text on disk -> `convert --parser device --window-mb N --compact-windows
--output-format mcircuit-bincode`, then a streamed proof of the converted file (`--stream --parser device`) beside the streamed proof
of the text with `--compact-windows`, in turn; the proofs are checked to be the same bytes."""
import argparse
import ctypes as C
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402

from bincode_bench import timed, timed_alternating  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gates", type=int, default=0, help="about this many gates (0: the headline circuit, 65536 x 153)")
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--window-ops", default="4194304,262144", help="comma-separated records per feed of the windowed writers")
    ap.add_argument("--window-mb", default="64", help="comma-separated window sizes in MiB of the chain")
    ap.add_argument("--no-dumps", action="store_true", help="leave out the one call of numpy's bristol.dumps")
    ap.add_argument("--no-chain", action="store_true")
    ap.add_argument("--parent-lib", default="", help="another commit's libreverie_amd.so: its whole-list program-file writer in turn with this tree's")
    a = ap.parse_args()
    window_ops = [int(x) for x in a.window_ops.split(",") if x]
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
    gates = np.ascontiguousarray(prog[:-2 * k])
    n_in = int(np.count_nonzero(gates["opcode"] == 0))
    ctx = rv.Context.default()
    L = _lib.lib()
    REC = OP_DTYPE.itemsize
    d_prog = torch.from_numpy(np.frombuffer(prog.tobytes(), np.uint8).copy()).cuda()
    d_gates = d_prog[:len(gates) * REC]
    rec = {"gates": st["gates"], "n_ops": len(prog), "runs": a.runs}

    # ---- Bristol text ----
    def host_bristol():
        out, n = C.c_void_p(), C.c_size_t()
        _lib.check(L.rv_bristol_write(C.c_void_p(gates.ctypes.data), C.c_size_t(len(gates)), C.c_uint64(0), C.c_uint64(k), C.byref(out), C.byref(n)))
        data = C.string_at(out, n.value)
        L.rv_free(out)
        return data

    text, t_host = timed(host_bristol, a.runs)
    n_wires = int(text.split(b"\n", 1)[0].split()[1])
    d_text = torch.empty(len(text), dtype=torch.uint8, device="cuda")

    def device_bristol():
        n = C.c_size_t()
        _lib.check(L.rv_bristol_write_device(ctx.handle, C.c_void_p(d_gates.data_ptr()), C.c_size_t(len(gates)), C.c_uint64(0), C.c_uint64(k),
                                             C.c_void_p(d_text.data_ptr()), C.c_size_t(d_text.numel()), C.byref(n)))
        return int(n.value)

    size, t_dev = timed(device_bristol, a.runs)
    rec.update({"text_bytes": len(text), "bristol_host_write": t_host, "bristol_device_write": t_dev,
                "bristol_writers_agree": size == len(text) and d_text.cpu().numpy().tobytes() == text})
    if not a.no_dumps:
        t0 = time.perf_counter()
        same = bristol.dumps(gates, k) == text
        rec.update({"bristol_numpy_dumps_ms": (time.perf_counter() - t0) * 1e3, "host_writer_equals_dumps": bool(same)})

    def windowed(kind, per_feed, keep=None):
        """the list through one windowed writer, `per_feed` records a feed, every feed into one buffer; keep: receives all bytes"""
        n_ops, ops = (len(gates), d_gates) if kind == "bristol" else (len(prog), d_prog)
        w, piece = C.c_void_p(), _lib.WriterPiece()
        if kind == "bristol":
            _lib.check(L.rv_bristol_writer_begin(ctx.handle, C.c_uint64(n_ops), C.c_uint64(n_in), C.c_uint64(n_wires), C.c_uint64(k), C.byref(w)))
            feed, finish, destroy = L.rv_bristol_writer_feed, L.rv_bristol_writer_finish, L.rv_bristol_writer_destroy
        else:
            _lib.check(L.rv_program_writer_begin(ctx.handle, C.c_uint64(n_ops), C.byref(w)))
            feed, finish, destroy = L.rv_program_writer_feed, L.rv_program_writer_finish, L.rv_program_writer_destroy
        try:
            for at in range(0, n_ops, per_feed):
                n = min(per_feed, n_ops - at)
                _lib.check(feed(w, C.c_void_p(ops.data_ptr() + at * REC), C.c_size_t(n), 1, C.c_void_p(w_buf.data_ptr()), C.c_size_t(w_buf.numel()),
                                C.byref(piece)))
                if keep is not None:
                    keep[piece.file_off:piece.file_off + piece.bytes] = w_buf[:piece.bytes]
            _lib.check(finish(w))
        finally:
            destroy(w)
        return int(piece.file_off + piece.bytes)

    def windows_of(kind, whole_ms, want):
        out = {}
        n_ops = len(gates) if kind == "bristol" else len(prog)
        for per_feed in window_ops:
            keep = torch.zeros(len(want), dtype=torch.uint8, device="cuda")
            ok = windowed(kind, per_feed, keep) == len(want) and keep.cpu().numpy().tobytes() == want
            del keep
            _, t = timed(lambda: windowed(kind, per_feed), a.runs)
            feeds = -(-n_ops // per_feed)
            out[str(per_feed)] = dict(t, feeds=feeds, same_bytes=bool(ok), ms_per_feed=(t["ms"] - whole_ms) / feeds)
        return out

    w_buf = torch.empty(96 + 41 * max(window_ops + [1]), dtype=torch.uint8, device="cuda")
    rec["bristol_windows"] = windows_of("bristol", t_dev["ms"], text)
    del d_text

    # ---- program files ----
    from reverie_amd import program_file

    data = program_file.dumps(prog)
    d_out = torch.empty(len(data), dtype=torch.uint8, device="cuda")

    def program_write(lib, handle):
        n = C.c_size_t()
        rc = lib.rv_program_to_bincode_device(handle, C.c_void_p(d_prog.data_ptr()), C.c_size_t(len(prog)), C.c_void_p(d_out.data_ptr()),
                                              C.c_size_t(d_out.numel()), C.byref(n))
        assert rc == 0, rc
        return int(n.value)

    size, t_pw = timed(lambda: program_write(L, ctx.handle), a.runs)
    rec.update({"file_bytes": len(data), "program_device_write": t_pw, "program_writers_agree": size == len(data) and d_out.cpu().numpy().tobytes() == data})
    if a.parent_lib:
        P = C.CDLL(a.parent_lib)
        p_ctx, fresh = C.c_void_p(), rv.Context(ctx.device)  # (a context of its own for each side: the same empty arena)
        P.rv_ctx_create.argtypes, P.rv_program_to_bincode_device.argtypes = [C.c_int, C.POINTER(C.c_void_p)], _lib.ARGTYPES["rv_program_to_bincode_device"]
        assert P.rv_ctx_create(ctx.device, C.byref(p_ctx)) == 0
        d_out.zero_()
        same = program_write(P, p_ctx) == len(data) and d_out.cpu().numpy().tobytes() == data
        sides = {"this": lambda: program_write(L, fresh.handle), "parent": lambda: program_write(P, p_ctx)}
        t = timed_alternating(sides, a.runs)
        t2 = timed_alternating(dict(reversed(list(sides.items()))), a.runs)  # ... and with the other side first
        rec["program_write_alt"] = dict(t, parent_same_bytes=bool(same), parent_first=t2)
    rec["program_windows"] = windows_of("program", t_pw["ms"], data)
    del d_out, w_buf
    print(json.dumps(rec), flush=True)
    if a.no_chain:
        return

    # ---- end to end: text on disk -> compacted program file, then streamed proofs of both ----
    from reverie_amd import __main__ as cli
    from reverie_amd import stream

    seeds = np.arange(4096, dtype=np.uint32).astype(np.uint8).reshape(256, 16)
    del d_prog
    with tempfile.TemporaryDirectory() as tmp:
        src, exp_path, out = os.path.join(tmp, "ssa.txt"), os.path.join(tmp, "expected.txt"), os.path.join(tmp, "compacted.bin")
        open(src, "wb").write(text)
        open(exp_path, "w").write("".join(map(str, exp.tolist())))
        for mb in [int(x) for x in a.window_mb.split(",") if x]:
            args = ["--operation", "convert", "--program-path", src, "--expected-outputs-path", exp_path, "--parser", "device", "--window-mb", str(mb),
                    "--compact-windows", "--output-path", out, "--output-format", "mcircuit-bincode"]
            _, t_conv = timed(lambda: cli.main(args), a.runs)
            proofs = {}

            def prove(name, pieces_of):
                wc_s, pieces = pieces_of()
                proofs[name] = bytes(stream.prove_streaming_pieces(pieces, wit, [], wc_s, seeds=seeds, ctx=ctx, device_compile=True)[0])

            fns = {"converted_file": lambda: prove("file", lambda: cli.stream_pieces(out, "mcircuit-bincode", "device", mb)),
                   "text_compact_windows": lambda: prove("text", lambda: cli.stream_pieces(src, "bristol", "device", mb, exp_path, in_windows=True))}
            t = timed_alternating(fns, a.runs)
            print(json.dumps({"chain_window_mb": mb, "convert": t_conv, "converted_bytes": os.path.getsize(out), "stream_proof": t,
                              "same_proof": proofs["file"] == proofs["text"]}), flush=True)


if __name__ == "__main__":
    main()
