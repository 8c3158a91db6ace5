"""Witness text on the GPU (rv_witness_parse_device, rv_witness_reader_*, rv_witness_write_device) beside the host
parsers and writers, and a proof from a witness file through `--witness-parser host|device`.

    python tools/witness_bench.py [--sizes 4096,67108864,1073741824] [--runs 5] [--window-mb 64,4] [--no-numpy] [--no-chain]

For each size: a text of that many bytes of '0' / '1' with a line feed every 64 bits.  One JSON line per size with, each the median
of --runs calls after one warm-up, with min and max: numpy's `parse_witness` (--no-numpy leaves it out), the host rv_witness_parse,
rv_witness_parse_device from host bytes and from a GPU tensor (into one buffer), the windowed reader at --window-mb MiB per feed
from host bytes (windows no smaller than the text are left out), the host rv_witness_write and rv_witness_write_device.  Every
parser and writer is checked once against the host definition.  The chain (--no-chain leaves it out): AES-128 as a Bristol file
and a 256-bit witness file, `--operation prove` with `--witness-parser host` and `device` in turn."""
import argparse
import ctypes as C
import json
import os
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402

from bincode_bench import timed, timed_alternating  # noqa: E402


def make_text(size: int) -> np.ndarray:
    rng = np.random.default_rng(size)
    a = rng.integers(0x30, 0x32, size, dtype=np.uint8)
    a[64::65] = 10
    return a


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="4096,67108864,1073741824", help="comma-separated text sizes in bytes")
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--window-mb", default="64,4", help="comma-separated window sizes in MiB of the windowed reader")
    ap.add_argument("--no-numpy", action="store_true", help="leave out numpy's parse_witness")
    ap.add_argument("--no-chain", action="store_true")
    a = ap.parse_args()
    import torch

    import reverie_amd as rv
    from reverie_amd import _lib, witness

    ctx = rv.Context.default()
    L = _lib.lib()
    for size in [int(x) for x in a.sizes.split(",") if x]:
        text = make_text(size)
        p_text = C.c_void_p(text.ctypes.data)
        n = C.c_size_t()
        rec = {"text_bytes": size, "runs": a.runs}
        bits = np.empty(size, np.uint8)

        def host_parse():
            _lib.check(L.rv_witness_parse(p_text, C.c_size_t(size), C.c_void_p(bits.ctypes.data), C.c_size_t(size), C.byref(n)))
            return int(n.value)

        n_bits, rec["host_parse"] = timed(host_parse, a.runs)
        rec["bits"] = n_bits
        if not a.no_numpy:
            got, rec["numpy_parse_witness"] = timed(lambda: witness.parse_witness(text.data), a.runs)
            rec["host_equals_numpy"] = bool(len(got) == n_bits and (got == bits[:n_bits]).all())
            del got
        d_text = torch.from_numpy(text).cuda()
        d_bits = torch.empty(size, dtype=torch.uint8, device="cuda")

        def device_parse(ptr, on_device, length=size, at=0):
            _lib.check(L.rv_witness_parse_device(ctx.handle, C.c_void_p(ptr), C.c_size_t(length), C.c_int(on_device), C.c_void_p(d_bits.data_ptr() + at),
                                                 C.c_size_t(size - at), C.byref(n), None, C.c_size_t(0), None))
            return int(n.value)

        got, rec["device_parse_from_host"] = timed(lambda: device_parse(text.ctypes.data, 0), a.runs)
        same = got == n_bits and bool((d_bits[:n_bits].cpu().numpy() == bits[:n_bits]).all())
        d_bits.zero_()
        got, rec["device_parse_from_gpu"] = timed(lambda: device_parse(d_text.data_ptr(), 1), a.runs)
        rec["device_equals_host"] = same and got == n_bits and bool((d_bits[:n_bits].cpu().numpy() == bits[:n_bits]).all())

        def windowed(window):
            h, at = C.c_void_p(), 0
            _lib.check(L.rv_witness_reader_begin(ctx.handle, C.byref(h)))
            try:
                for off in range(0, size, window):
                    m = min(window, size - off)
                    _lib.check(L.rv_witness_reader_feed(h, C.c_void_p(text.ctypes.data + off), C.c_size_t(m), 0, C.c_void_p(d_bits.data_ptr() + at),
                                                        C.c_size_t(size - at), C.byref(n)))
                    at += int(n.value)
            finally:
                L.rv_witness_reader_destroy(h)
            return at

        rec["reader_from_host"] = {}
        for mb in [int(x) for x in a.window_mb.split(",") if x]:
            if (mb << 20) >= size:
                continue
            d_bits.zero_()
            got, t = timed(lambda: windowed(mb << 20), a.runs)
            ok = got == n_bits and bool((d_bits[:n_bits].cpu().numpy() == bits[:n_bits]).all())
            rec["reader_from_host"][str(mb)] = dict(t, feeds=-(-size // (mb << 20)), same_bits=ok)

        # the writers, on the text's own bits
        out = np.empty(size + 1, np.uint8)

        def host_write():
            _lib.check(L.rv_witness_write(C.c_void_p(bits.ctypes.data), C.c_size_t(n_bits), C.c_uint64(64), C.c_void_p(out.ctypes.data), C.c_size_t(out.size),
                                          C.byref(n)))
            return int(n.value)

        length, rec["host_write"] = timed(host_write, a.runs)
        d_src = d_bits[:n_bits].clone()
        d_out = torch.empty(length, dtype=torch.uint8, device="cuda")

        def device_write():
            _lib.check(L.rv_witness_write_device(ctx.handle, C.c_void_p(d_src.data_ptr()), C.c_size_t(n_bits), C.c_uint64(64), C.c_void_p(d_out.data_ptr()),
                                                 C.c_size_t(length), C.byref(n)))
            return int(n.value)

        got, rec["device_write"] = timed(device_write, a.runs)
        rec["writers_agree"] = got == length and bool((d_out.cpu().numpy() == out[:length]).all())
        print(json.dumps(rec), flush=True)
        del d_text, d_bits, d_src, d_out, text, bits, out
    if a.no_chain:
        return

    # ---- file to proof: AES-128 (the 256-bit witness is a text of about 4 lines) ----
    import bristol_gen
    from reverie_amd import __main__ as cli

    with tempfile.TemporaryDirectory() as tmp:
        src, wit, proof = os.path.join(tmp, "aes128.txt"), os.path.join(tmp, "witness.txt"), os.path.join(tmp, "proof.bin")
        open(src, "w").write(bristol_gen.aes128())
        open(wit, "wb").write(witness.dumps(np.random.default_rng(1).integers(0, 2, 256, dtype=np.uint8), 64))
        devnull = open(os.devnull, "w")

        def prove(parser):
            stdout, sys.stdout = sys.stdout, devnull
            try:
                assert cli.main(["--operation", "prove", "--program-path", src, "--witness-path", wit, "--proof-path", proof, "--witness-parser", parser]) == 0
            finally:
                sys.stdout = stdout

        t = timed_alternating({"host": lambda: prove("host"), "device": lambda: prove("device")}, a.runs)
        print(json.dumps({"chain": "aes128 prove, witness file to proof file", "witness_parser": t}), flush=True)


if __name__ == "__main__":
    main()
