"""The mixed workload of the B2A measurements (tools/compile_device_bench.py and tools/stream_bench.py, --compiler device-b2a): the
half-and-half mixture of configs 4 and 5 in alternating runs of 4096 ops, and behind it a band of `n_b2a` B2A ops that bridge GF(2)
wires into the Z64 half -- B2A number j converts the 64 GF(2) wires from 64 j on (wrapping over the wires the GF(2) half wrote) into
a Z64 wire of its own, and one Z64 Add folds that wire into the Z64 half."""
import numpy as np

import circuits
from reverie_amd.ops import B2A, Z64, program


def mixed_b2a(n_b2a=4096, n_mul=500_000, recycle=False):
    """-> (program, GF(2) witness, Z64 witness, (z64_wires, gf2_wires))"""
    p5, w64, wc5, _ = circuits.layered_z64(n_mul=n_mul, recycle=recycle)
    p4, w2, wc4, _ = circuits.layered_gf2(layers=max(1, len(p5) // 65536), recycle=recycle)
    # (whole programs of both halves: a cut half would lose the asserted tail)
    mix = np.empty(len(p4) + len(p5), p5.dtype)
    run = 4096
    a4 = a5 = at = 0
    while at < len(mix):
        k = min(run, len(p4) - a4)
        mix[at:at + k] = p4[a4:a4 + k]
        at, a4 = at + k, a4 + k
        k = min(run, len(p5) - a5)
        mix[at:at + k] = p5[a5:a5 + k]
        at, a5 = at + k, a5 + k
    z0, g = wc5[0], wc4[1]
    band = []
    for j in range(n_b2a):
        band.append(B2A(z0 + j, (64 * j) % (g - 63)))
        band.append(Z64.Add(z0 + j, z0 + j, j % z0))
    prog = np.concatenate([mix, program(band)]) if band else mix
    return prog, list(w2), list(w64), (z0 + n_b2a, g)
