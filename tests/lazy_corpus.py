"""The programs the lazy-sum (RV_COMPILE_WHOLE_PROVER) device compile is checked on: the random corpus of test_gpu_compile_device.py
(same seed and parameters) and one crafted program that holds every case of the materialisation rule.  Shared by
test_compile_device_lazy_host.py, which pins on the host compiler alone that the corpus exercises the rule, and
test_gpu_compile_device_lazy.py, which compares the two compilers on it."""
import ctypes as C
import functools

import numpy as np

import circuits
from reverie_amd.ops import GF2, program

RV_COMPILE_WHOLE_PROVER, RV_COMPILE_KEEP_WIRES, RV_COMPILE_DEVICE = 1, 2, 4


@functools.lru_cache(maxsize=None)
def random_programs():
    """240 circuits.random_gf2 programs -> [(prog, witness, wire_counts)]; built once, never changed"""
    rng = np.random.default_rng(0xC0DE)
    progs = []
    for _ in range(240):
        n_wires = int(rng.choice([3, 6, 12, 40, 150, 600]))
        n_gates = int(rng.choice([20, 120, 400, 1500, 4000]))
        prog, wit, wc = circuits.random_gf2(rng, n_in=int(rng.integers(1, 24)), n_gates=n_gates, n_wires=n_wires)
        progs.append((prog, wit, wc))
    return tuple(progs)


CRAFTED_WITNESS = [1, 1, 0, 1, 0, 1, 0, 1]  # a .. h
# what the host rule makes of crafted_program() with RV_COMPILE_WHOLE_PROVER: the sums on wires 11, 14, 18, 21, 22 and 29 become
# G_XORK gates (of 2, 3, 6, 4, 3 and 2 rows), every other sum stays symbolic or is dropped
CRAFTED_MATERIALISED = 6
CRAFTED_XORK_ROWS = 2 + 3 + 6 + 4 + 3 + 2


def crafted_program():
    """-> (prog, witness, wire_counts).  Wires 0-7: Inputs a .. h (PRG rows 0-7), 8: Random r (row 8), 9: m = a & b (a Mul's row);
    36 and 37 are temporaries and 39 takes every Mul result nobody reads (wire reuse); 38 is never written.  A sum of n rows read
    f times stays symbolic when n <= 1, or n <= 3 and f (n - 1) <= n + 1."""
    T, U, D, N = 36, 37, 39, 38
    ops = [GF2.Input(i) for i in range(8)] + [GF2.Random(8), GF2.Mul(9, 0, 1)]
    # wire 10: a two-row sum read exactly 3 times -> symbolic
    ops += [GF2.Add(10, 0, 1), GF2.Mul(D, 10, 2), GF2.Mul(D, 10, 3), GF2.Mul(D, 10, 4)]
    # wire 11: a two-row sum read 4 times -> materialised (class 2); wire 12: AddConst on its computed row
    ops += [GF2.Add(11, 2, 3), GF2.Mul(D, 11, 0), GF2.Mul(D, 11, 1), GF2.Mul(D, 11, 4), GF2.AddConst(12, 11, 1)]
    # wire 13: e ^ f ^ g, a three-row sum read 2 times (here and by wire 18) -> symbolic
    ops += [GF2.Add(T, 4, 5), GF2.Add(13, T, 6), GF2.Mul(D, 13, 0)]
    # wire 14: f ^ g ^ h, a three-row sum read 3 times -> materialised (na = 3, class 3)
    ops += [GF2.Add(T, 5, 6), GF2.Sub(14, T, 7), GF2.Mul(D, 14, 0), GF2.Mul(D, 14, 1), GF2.Mul(D, 14, 2)]
    # wire 15: (a ^ b) ^ (b ^ c) cancels to a ^ c; wire 16: x ^ x, the constant 0, and AssertZero of a constant
    ops += [GF2.Add(T, 0, 1), GF2.Add(U, 1, 2), GF2.Add(15, T, U), GF2.Mul(D, 15, 3), GF2.Add(16, 15, 15), GF2.AssertZero(16)]
    # wire 17: a ^ b ^ c read 2 times: AssertZero of a three-row form (it holds: 1 ^ 1 ^ 0) and wire 18
    ops += [GF2.Add(T, 0, 1), GF2.Add(17, T, 2), GF2.AssertZero(17)]
    # wire 18: two three-row forms with no common row -> one G_XORK of 6 rows (na = 3, nb = 3)
    ops += [GF2.Add(18, 13, 17), GF2.Mul(D, 18, 8)]
    # wire 21: a ^ d ^ m plus d ^ h ^ r, one common row -> a G_XORK of 4 rows (nb = 1); Input, Random and Mul rows in one form
    ops += [GF2.Add(T, 0, 3), GF2.Add(19, T, 9), GF2.Add(T, 3, 7), GF2.Add(20, T, 8), GF2.Add(21, 19, 20), GF2.Mul(D, 21, 1)]
    # wire 22: c ^ e ^ h ^ 1 read 3 times -> materialised with the constant in the gate (ca = 1)
    ops += [GF2.Add(T, 4, 7), GF2.AddConst(U, T, 1), GF2.Add(22, U, 2), GF2.Mul(D, 22, 0), GF2.Mul(D, 22, 1), GF2.Mul(D, 22, 3)]
    # wire 25: a Mul of a three-row form with constant 1 (wire 23) and a two-row form (wire 24)
    ops += [GF2.Add(T, 5, 7), GF2.Add(U, T, 3), GF2.SubConst(23, U, 1), GF2.Add(24, 1, 6), GF2.Mul(25, 23, 24)]
    # wire 27: a Mul by a pure constant
    ops += [GF2.Const(26, 1), GF2.Mul(27, 26, 0)]
    # wire 28: a dead sum of 3 rows (dropped; its read of the temporary still counts)
    ops += [GF2.Add(T, 0, 4), GF2.Add(28, T, 6)]
    # wire 29: a two-row sum with 3 live reads and one by the dead sum on wire 30 -> 4 reads, materialised
    ops += [GF2.Add(29, 2, 5), GF2.Mul(D, 29, 0), GF2.Mul(D, 29, 1), GF2.Mul(D, 29, 4), GF2.Add(30, 29, 7)]
    # wire 31: a sum with the never-written wire 38 (one row); then a Mul whose second operand is that wire
    ops += [GF2.Add(31, N, 0), GF2.Mul(D, 31, N)]
    # wire 33: e ^ r ^ (computed row of wire 11): Input and Random rows sort before the computed row
    ops += [GF2.Add(32, 11, 8), GF2.Add(33, 32, 4), GF2.Mul(D, 33, 14)]
    # wire 34: AddConst / SubConst / MulConst 1 on the three-row form b ^ d ^ f; wire 35: MulConst 0 of it, AssertZero of a constant
    ops += [GF2.Add(T, 1, 3), GF2.Add(U, T, 5), GF2.AddConst(34, U, 1), GF2.SubConst(34, 34, 1), GF2.MulConst(34, 34, 1),
            GF2.Mul(D, 34, 0), GF2.MulConst(35, 34, 0), GF2.AssertZero(35)]
    return program(ops), list(CRAFTED_WITNESS), (0, 40)


def corpus():
    """every program of the corpus, the crafted one last"""
    return list(random_programs()) + [crafted_program()]


def compile_info(prog, wc, flags):
    """rv_hook_compile_info (host only) -> (status, CircuitInfo)"""
    from reverie_amd import _lib

    info = _lib.CircuitInfo()
    rc = _lib.lib().rv_hook_compile_info(prog.ctypes.data_as(C.c_void_p), C.c_size_t(len(prog)), C.c_size_t(wc[0]), C.c_size_t(wc[1]),
                                         C.c_uint32(flags), C.c_size_t(0), C.byref(info))
    return rc, info
