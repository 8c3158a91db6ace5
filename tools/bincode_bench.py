"""Program files on the GPU (rv_program_from_bincode_device / rv_program_to_bincode_device) beside the host reader and
writer, on the two benchmark circuits written as bincode(Vec<CombineOperation>) by program_file.dumps.

    python tools/bincode_bench.py [--circuits gf2,z64] [--runs 5] [--no-chain] [--window-mb 64,4]

gf2: the 10^7-gate config-4 circuit (layered_gf2); z64: the 10^6-MUL config-5 circuit (layered_z64).  Both readers are checked once to
give the same records, both writers the same bytes.  One JSON line per circuit with, each the median of --runs calls after one
warm-up, with min and max: rv_program_from_bincode; rv_program_from_bincode_device from host bytes; the same from bytes in GPU memory
(the difference is the upload); rv_program_to_bincode and rv_program_to_bincode_device; and the chain from file bytes to proof --
host reader -> rv_circuit_compile -> rv_prove beside device reader (host bytes) -> rv_circuit_compile_device -> rv_prove.  The
baseline and the device path run in one process, on the same bytes.

--window-mb N[,N..]: the file read in windows of N MiB as well (rv_program_reader_*), from host bytes and from bytes in
GPU memory, the runs alternating with the whole-file device call's ("window_reads": {N: ...}, and "whole_read_*" for the whole-file
calls of the same alternation; the windows' records are checked once against the host reader's), and with the chain the file ->
streamed proof of `--stream --parser device --compiler device*` (a scan pass and two read passes over the file on disk;
"chain_stream": {N: ...}) beside file -> resident proof ("chain_device_alt": the same alternation)."""
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


def timed_alternating(fns: dict, runs):
    """-> {name: {median, min, max} in ms}: one warm-up each, then `runs` rounds that call every function once, in turn"""
    for fn in fns.values():
        fn()
    ts = {k: [] for k in fns}
    for _ in range(runs):
        for k, fn in fns.items():
            t0 = time.perf_counter()
            fn()
            ts[k].append((time.perf_counter() - t0) * 1e3)
    return {k: {"ms": sorted(v)[len(v) // 2], "ms_min_max": [min(v), max(v)]} for k, v in ts.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--circuits", default="gf2,z64")
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--no-chain", action="store_true", help="the readers and writers alone")
    ap.add_argument("--window-mb", default="", help="comma-separated window sizes in MiB: the windowed reader and the streamed chain beside the whole-file ones")
    a = ap.parse_args()
    windows_mb = [int(x) for x in a.window_mb.split(",") if x]
    import torch

    import circuits
    import reverie_amd as rv
    from reverie_amd import _lib, program_file
    from reverie_amd.ops import OP_DTYPE

    ctx = rv.Context.default()
    L = _lib.lib()
    seeds = np.arange(4096, dtype=np.uint32).astype(np.uint8).reshape(256, 16)
    for which in a.circuits.split(","):
        if which == "gf2":
            prog, wit, wc, st = circuits.layered_gf2()
            w2, w64 = wit, []
        else:
            prog, wit, wc, st = circuits.layered_z64()
            w2, w64 = [], wit
        data = program_file.dumps(prog)
        h_data = np.frombuffer(data, np.uint8)
        d_data = torch.from_numpy(h_data.copy()).cuda()
        n_ops = len(prog)
        d_ops = torch.empty((n_ops, OP_DTYPE.itemsize), dtype=torch.uint8, device="cuda")
        d_out = torch.empty((len(data),), dtype=torch.uint8, device="cuda")

        def host_read():
            ops, n = C.c_void_p(), C.c_size_t()
            _lib.check(L.rv_program_from_bincode(C.c_void_p(h_data.ctypes.data), C.c_size_t(h_data.size), C.byref(ops), C.byref(n)))
            out = np.frombuffer(C.string_at(ops, n.value * OP_DTYPE.itemsize), dtype=OP_DTYPE)
            L.rv_free(ops)
            return out

        def device_read(src, on_device):  # (the records' room is there: the C call alone)
            n, pi = C.c_size_t(), _lib.ProgramInfo()
            _lib.check(L.rv_program_from_bincode_device(ctx.handle, C.c_void_p(src), C.c_size_t(h_data.size), on_device, C.c_void_p(d_ops.data_ptr()),
                                                        C.c_size_t(n_ops), C.byref(n), C.byref(pi)))
            return int(n.value), (int(pi.z64_wires), int(pi.gf2_wires))

        def host_write():
            out, n = C.c_void_p(), C.c_size_t()
            _lib.check(L.rv_program_to_bincode(C.c_void_p(prog.ctypes.data), C.c_size_t(n_ops), C.byref(out), C.byref(n)))
            size = int(n.value)
            L.rv_free(out)
            return size

        def device_write():
            n = C.c_size_t()
            _lib.check(L.rv_program_to_bincode_device(ctx.handle, C.c_void_p(d_ops.data_ptr()), C.c_size_t(n_ops), C.c_void_p(d_out.data_ptr()),
                                                      C.c_size_t(d_out.numel()), C.byref(n)))
            return int(n.value)

        h_ops, t_host = timed(host_read, a.runs)
        (n_dev, d_wc), t_dev_host = timed(lambda: device_read(h_data.ctypes.data, 0), a.runs)
        d_ops.zero_()
        (_, _), t_dev_dev = timed(lambda: device_read(d_data.data_ptr(), 1), a.runs)
        same = n_dev == len(h_ops) and d_ops.cpu().numpy().tobytes() == h_ops.tobytes() and d_wc == tuple(int(x) for x in rv.ops.largest_wires(h_ops))
        _, t_hwrite = timed(host_write, a.runs)
        size, t_dwrite = timed(device_write, a.runs)
        rec = {"circuit": which, "n_ops": n_ops, "file_bytes": len(data), "runs": a.runs, "readers_agree": bool(same),
               "read_equals_generator": h_ops.tobytes() == prog.tobytes(), "writers_agree": size == len(data) and d_out.cpu().numpy().tobytes() == data,
               "host_read": t_host, "device_read_host_bytes": t_dev_host, "device_read_device_bytes": t_dev_dev,
               "host_write": t_hwrite, "device_write": t_dwrite}
        if not a.no_chain:
            def chain_host():
                ops = program_file.loads(data)
                return bytes(rv.Proof.new(rv.Circuit(ops, wc), w2, w64, seeds=seeds))

            def chain_device():
                ops, info = program_file.loads_device(h_data, device=ctx)
                return bytes(rv.Proof.new(rv.Circuit.from_device_ops(ops, wc, ctx, device_z64=which != "gf2"), w2, w64, seeds=seeds))

            p_host, t_chain_host = timed(chain_host, a.runs)
            p_dev, t_chain_dev = timed(chain_device, a.runs)
            rec.update({"chain_host": t_chain_host, "chain_device": t_chain_dev, "same_proof": p_host == p_dev})
        if windows_mb:
            import tempfile

            from reverie_amd import __main__ as cli
            from reverie_amd import stream

            def window_read(src, on_device, mb, check=False):
                """the whole file through one reader in windows of mb MiB, every window's records into one window buffer"""
                w, at, n_out = mb << 20, 0, 0
                buf = torch.empty((min(w, h_data.size) // 16 + 1, OP_DTYPE.itemsize), dtype=torch.uint8, device="cuda")
                r, piece = C.c_void_p(), _lib.ProgramPiece()
                _lib.check(L.rv_program_reader_begin(ctx.handle, C.c_uint64(h_data.size), C.byref(r)))
                try:
                    while at < h_data.size:
                        n = min(w, h_data.size - at)
                        _lib.check(L.rv_program_reader_feed(r, C.c_void_p(src + at), C.c_size_t(n), on_device, C.c_void_p(buf.data_ptr()),
                                                            C.c_size_t(buf.shape[0]), C.byref(piece)))
                        if check:
                            d_ops[piece.first_op:piece.first_op + piece.n_ops] = buf[:piece.n_ops]
                        at, n_out = at + n, n_out + int(piece.n_ops)
                    pi = _lib.ProgramInfo()
                    _lib.check(L.rv_program_reader_finish(r, C.byref(pi)))
                finally:
                    L.rv_program_reader_destroy(r)
                return n_out, (int(pi.z64_wires), int(pi.gf2_wires))

            agree = True
            for mb in windows_mb:
                for src, on_device in ((h_data.ctypes.data, 0), (d_data.data_ptr(), 1)):
                    d_ops.zero_()
                    n_w, wc_w = window_read(src, on_device, mb, check=True)
                    agree &= n_w == len(h_ops) and wc_w == d_wc and d_ops.cpu().numpy().tobytes() == h_ops.tobytes()
            fns = {"whole_read_host_bytes": lambda: device_read(h_data.ctypes.data, 0), "whole_read_device_bytes": lambda: device_read(d_data.data_ptr(), 1)}
            for mb in windows_mb:
                fns[f"host_bytes@{mb}"] = lambda mb=mb: window_read(h_data.ctypes.data, 0, mb)
                fns[f"device_bytes@{mb}"] = lambda mb=mb: window_read(d_data.data_ptr(), 1, mb)
            t = timed_alternating(fns, a.runs)
            rec.update({"windows_agree": bool(agree), "whole_read_host_bytes": t.pop("whole_read_host_bytes"),
                        "whole_read_device_bytes": t.pop("whole_read_device_bytes"), "window_reads": t})
            if not a.no_chain:
                with tempfile.TemporaryDirectory() as tmp:
                    path = os.path.join(tmp, "program.bin")
                    with open(path, "wb") as f:
                        f.write(data)
                    proofs = {}

                    def chain_stream(mb):
                        wc_s, pieces = cli.stream_pieces(path, "mcircuit-bincode", "device", mb)
                        proofs[mb] = bytes(stream.prove_streaming_pieces(pieces, w2, w64, wc_s, seeds=seeds, ctx=ctx, device_compile=True,
                                                                         device_z64=which != "gf2")[0])

                    def chain_file():  # (the file on disk, memory-mapped as the command line does)
                        ops, wc_f = cli.load_program_device(path, None, "mcircuit-bincode")
                        proofs["resident"] = bytes(rv.Proof.new(rv.Circuit.from_device_ops(ops, wc_f, ctx, device_z64=which != "gf2"), w2, w64, seeds=seeds))

                    fns = {"chain_device_alt": chain_file, **{str(mb): (lambda mb=mb: chain_stream(mb)) for mb in windows_mb}}
                    t = timed_alternating(fns, a.runs)
                    rec.update({"chain_device_alt": t.pop("chain_device_alt"), "chain_stream": t,
                                "stream_same_proof": all(p == proofs["resident"] for p in proofs.values())})
        print(json.dumps(rec), flush=True)
        del d_data, d_ops, d_out


if __name__ == "__main__":
    main()
