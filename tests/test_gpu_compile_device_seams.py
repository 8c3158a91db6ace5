"""The device compiler where its drivers hand over to each other (csrc/compile_dev.hip: the split of a mixed list, the GF(2) levels,
the Z64 levels, the GF(2) tables, the Z64 tables): op lists in which one of the two domains' lists is empty or holds nothing but a
B2A's expansion, as whole programs in both forms and as a chunk with a non-zero start, against the host compiler field by field; and
the per-phase laps of a mixed and of a GF(2)-only compile."""
import ctypes as C
import math

import pytest

from reverie_amd.ops import B2A, GF2, SizeHint, Z64, program
from test_gpu_compile_device_z64 import _L, compare, compare_chunk

pytestmark = pytest.mark.gpu

RV_COMPILE_WHOLE_PROVER, RV_COMPILE_DEVICE, RV_COMPILE_DEVICE_Z64, RV_COMPILE_DEVICE_B2A = 1, 4, 8, 32
DEVB = RV_COMPILE_DEVICE | RV_COMPILE_DEVICE_Z64 | RV_COMPILE_DEVICE_B2A
START = (127, 1, 5, 3, 17, 2)  # mask_phase, mask64_phase, on0, pre0, on64, pre64: every counter of a piece starts off zero

# name -> (ops, (z64_wires, gf2_wires))
LISTS = {
    "hints_only": ([SizeHint(2, 3), SizeHint(0, 0), SizeHint(2, 3)], (2, 3)),  # both domains' lists are empty
    "b2a_alone": ([B2A(0, 0)], (1, 64)),  # its 64 source wires are never written
    "inputs_b2a": ([GF2.Input(i) for i in range(64)] + [B2A(0, 0)], (1, 64)),  # the Z64 list is the B2A's record alone
    "b2a_z64": ([B2A(0, 0), Z64.Input(1), Z64.Mul(2, 0, 1), Z64.AddConst(0, 2, 5), Z64.AssertZero(3)], (4, 64)),  # the GF(2) list is the expansion alone
    "z64_hint": ([Z64.Input(0), SizeHint(2, 0), Z64.Mul(1, 0, 0), Z64.AssertZero(1)], (2, 0)),  # the GF(2) list is empty
}
# (host status, path, diff) of each list in each form, recorded from the compiler before its drivers were untangled.  A list of
# SizeHints alone is compiled on the device (the empty GF(2) list of a mixed compile, unlike an empty program); a lone adder is deep and
# narrow (lazy_forms_pay), so its plain form is the host compiler's; every chunk and every forced lazy-sum form is the device's.
EXPECT = {
    "hints_only": {"plain": (0, 1, 0), "whole_prover": (0, 1, 0), "chunk": (0, 1, 0)},
    "b2a_alone": {"plain": (0, 0, 0), "whole_prover": (0, 1, 0), "chunk": (0, 1, 0)},
    "inputs_b2a": {"plain": (0, 0, 0), "whole_prover": (0, 1, 0), "chunk": (0, 1, 0)},
    "b2a_z64": {"plain": (0, 0, 0), "whole_prover": (0, 1, 0), "chunk": (0, 1, 0)},
    "z64_hint": {"plain": (0, 1, 0), "whole_prover": (0, 1, 0), "chunk": (0, 1, 0)},
}


def run_form(name, form):
    ops, wc = LISTS[name]
    prog = program(ops)
    if form == "chunk":
        return compare_chunk(prog, wc, START, DEVB)
    return compare(prog, wc, DEVB | (RV_COMPILE_WHOLE_PROVER if form == "whole_prover" else 0))


@pytest.mark.parametrize("form", ["plain", "whole_prover", "chunk"])
@pytest.mark.parametrize("name", list(LISTS))
def test_seam_lists(name, form):
    rc, path, diff = run_form(name, form)
    want_rc, want_path, want_diff = EXPECT[name][form]
    assert diff == want_diff == 0, (name, form, rc, path, diff)
    assert rc == want_rc, (name, form, rc, path, diff)
    assert path == want_path, (name, form, rc, path, diff)


def _laps():
    laps, z = (C.c_double * 6)(), C.c_double()
    assert _L().rv_hook_compile_device_laps(laps) == 0 and _L().rv_hook_compile_device_laps_z64(C.byref(z)) == 0
    return list(laps), z.value


def test_laps_of_a_mixed_and_a_gf2_compile():
    ops = LISTS["inputs_b2a"][0] + LISTS["b2a_z64"][0][1:] + [GF2.Mul(0, 0, 1), GF2.AssertZero(2)]
    assert compare(program(ops), (4, 64), DEVB | RV_COMPILE_WHOLE_PROVER) == (0, 1, 0)
    laps, z = _laps()
    assert all(math.isfinite(x) and x >= 0 for x in laps + [z]), (laps, z)
    assert z > 0 and sum(laps[:5]) > 0  # (the marks were recorded: the split and the Z64 steps take time)
    assert laps[5] >= 64  # (rounds: an adder's carry chain)
    gf2 = program([GF2.Input(0), GF2.Input(1), GF2.Mul(2, 0, 1), GF2.Add(3, 2, 0), GF2.AssertZero(3)])
    assert compare(gf2, (0, 4), RV_COMPILE_DEVICE) == (0, 1, 0)
    laps, z = _laps()
    assert all(math.isfinite(x) and x >= 0 for x in laps), laps
    assert z == 0
