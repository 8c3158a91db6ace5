"""tests/class_mix64.py on the host alone (rv_hook_z64_fused_levels, rv_hook_z64_fused_grid: no device): every spec
test_gpu_level_classes64.py runs must compile to exactly the (Mul, linear, other) counts it asks for, level by level, be eligible for
the fused path or not for the reason it is named for, and land in the branch of the launcher's grid arithmetic and in the regime of
the kernel's wavefront deal that it is named for -- the proof that the GPU tests aim where they say.  If a spec misses, the generator
or the spec is what changes."""
import ctypes as C

import numpy as np
import pytest

import class_mix64 as cm
from reverie_amd.ops import Z64, program

CUS = (256, 8)
CONFIGS = ((16, 4), (16, 2), (16, 1), (8, 1))  # (QW, quad groups): whole proofs, shards of 128, 64 and 32 repetitions


@pytest.fixture(scope="module", params=CUS)
def specs(request):
    return request.param, cm.all_specs(request.param)


def test_every_spec_compiles_to_its_counts_and_eligibility(specs):
    cus, table = specs
    for name, spec in table.items():
        prog, wit, wc, want = cm.build(spec)
        got, why = cm.fused_levels(prog, wc)
        assert got == want, name
        assert why == spec.why, name
        assert want[:len(spec.levels)] == [cm.bounds(lv) for lv in spec.levels], name  # (what was asked for; then the sink)
        assert len(want) <= len(spec.levels) + 3 and all(w[0] == 0 for w in want[len(spec.levels):]), name
        assert len(wit) == spec.levels[0][7], name
        assert all(sum(w) for w in want), name  # (no empty level: one launch per level)


def test_a_random_gate_makes_a_circuit_ineligible():
    prog, wit, wc = cm.class_mix64(cm.MIXED, cm.SEED)
    assert cm.fused_levels(prog, wc)[1] == cm.ELIGIBLE
    with_random = np.concatenate([prog, program([Z64.Random(wc[0])])])
    levels, why = cm.fused_levels(with_random, (wc[0] + 1, 0))
    assert why == cm.WHY_GATE and levels == []
    # a Random gate in front shifts every Mul's mask pair as an Input would: the unsupported gate is the reason reported
    levels, why = cm.fused_levels(np.concatenate([program([Z64.Random(wc[0])]), prog]), (wc[0] + 1, 0))
    assert why == cm.WHY_GATE
    assert cm.fused_levels(program([]), (1, 0)) == ([], 4)  # no Z64 gate at all


def test_grid_of_every_level_covers_it(specs):
    """chunks * per >= n for every class of every level of every spec, every `per` a multiple of its rounding unit, on every launch
    shape; an empty level or no quad group launches nothing"""
    cus, table = specs
    for name, spec in table.items():
        for counts in cm.build(spec)[3]:
            for qw, n_qg in CONFIGS:
                jw = 64 // qw
                chunks, mul_per, lin_per, oth_per, bias = cm.fused_grid(qw, n_qg, cus, *counts)
                assert bias == cm.LIN_BIAS and chunks >= 1, (name, counts)
                for n, per, unit in zip(counts, (mul_per, lin_per, oth_per), (jw, jw, 8 * jw)):
                    assert chunks * per >= n and per % unit == 0, (name, counts, qw, n_qg)
                    assert (chunks - 1) * (per - unit) < n or n == 0 or per == unit, (name, counts, qw, n_qg)  # (no more than rounding)
                assert [sum(c) for c in zip(*cm.chunk_counts(counts, (chunks, mul_per, lin_per, oth_per)))] == list(counts)
    assert cm.fused_grid(16, 4, cus, 0, 0, 0)[0] == 0 and cm.fused_grid(16, 0, cus, 5, 5, 5)[0] == 0
    assert cm.fused_grid(16, 1, 0, 1 << 20, 0, 0)[0] == cm.machine_cus()


def test_chunk_specs_take_the_branch_they_are_named_for(specs):
    cus, _ = specs
    seen = set()
    for qw, n_qg in ((16, 4), (8, 1)):
        for name, (levels, at, branch) in cm.chunk_specs(cus, qw, n_qg).items():
            got = cm.level_labels(cm.bounds(levels[at]), qw, n_qg, cus)[0]
            assert branch in got, (name, qw, got)
            seen |= got
    want = {"one-chunk", "two-chunks", "saturated", "at-per_qg", "mem>mul", "trailing-empty", "no-mul-allowance"}
    assert want <= seen, want - seen
    # the specs the GPU file runs are built for (16, 4): their branches at every launch shape are at least printed
    for name, (levels, at, branch) in cm.chunk_specs(cus).items():
        print(name, {cfg: sorted(cm.level_labels(cm.bounds(levels[at]), *cfg, cus)[0]) for cfg in CONFIGS})


def test_wavefront_deal_coverage(specs):
    """the (regime, x) pairs the deal specs hit: every pair there is, with every wavefront in the main loop (saturated specs, whole
    proofs) and with wavefronts that run the tail loop only (one chunk), at JW = 4 and at JW = 8"""
    cus, table = specs
    assert len(cm.DEAL_REGIMES) == 22 and not any(3 * x + 7 < 24 for x in (6, 7))  # (no "scarce" at x = 6, 7)
    main, tail = set(), {4: set(), 8: set()}
    for (reg, x), (m, n) in cm.deal_sat_specs(cus).items():
        deal = cm.level_labels((m, n, 0), 16, 4, cus)[1]
        assert {d[:2] for d in deal} == {(reg, x)} and not any(d[2] for d in deal), (reg, x, deal)
        main |= {d[:2] for d in deal}
    assert main == set(cm.DEAL_REGIMES)
    for jw, (qw, n_qg) in ((4, (16, 4)), (8, (8, 1))):
        for (reg, x), (m, n) in cm.DEAL_ONE_CHUNK[jw].items():
            br, deal, rem = cm.level_labels((m, n, 0), qw, n_qg, 256)
            assert br == {"one-chunk"} and deal == {(reg, x, x > 0)}, (jw, reg, x, br, deal)
            tail[jw].add((reg, x))
        for m, n in cm.DEAL_NO_LIN[jw]:
            wp = cm.wave_plan(m, n, jw)
            assert wp["TL"] == 0 and wp["regime"] in ("scarce", "equal") and not any(wp["LI"])
        want = {(r, x) for r, x in cm.DEAL_REGIMES if (r != "plenty" or x >= 3) and (r != "equal" or x >= 1)}
        assert tail[jw] == want, (jw, want ^ tail[jw])
    # TL = 1 and TL = 0 are among the scarce ones
    assert any(cm.wave_plan(m, n, 4)["TL"] == 1 for m, n in cm.DEAL_ONE_CHUNK[4].values())
    print("deal:", sorted(main), {jw: sorted(t) for jw, t in tail.items()})


def test_wave_plan_deals_every_step_once():
    """the transcription itself: the wavefronts' linear steps [l0s, l0s + LI) are disjoint and cover 0 .. TL - 1 (a label must at
    least be a sane one)"""
    for jw in (4, 8):
        for n_m in range(0, 20 * jw, 3):
            for n_l in range(0, 40 * jw, 5):
                wp = cm.wave_plan(n_m, n_l, jw)
                steps = sorted(s for w in range(8) for s in range(wp["l0s"][w], wp["l0s"][w] + wp["LI"][w]))
                assert steps == list(range(len(steps))) and len(steps) >= wp["TL"], (jw, n_m, n_l)
                assert sum(wp["MI"]) == wp["TM"]


def test_step_remainders_covered(specs):
    cus, table = specs
    for jw, cfg in ((4, (16, 4)), (8, (8, 1))):
        rem = set()
        for name, lv in cm.rem_specs(jw).items():
            rem |= cm.level_labels(cm.bounds(lv[2]), *cfg, cus)[2]
        want = {(c, r) for c, u in (("mul", jw), ("lin", jw), ("oth", 8 * jw)) for r in (1, u - 1)}
        assert want <= rem, (jw, want - rem)
        print("remainders:", jw, sorted(rem))


def test_operand_forms_values_and_orders_covered():
    forms, flags = cm.coverage(cm.ROTATION, cm.SEED)
    assert cm.WANT_FORMS <= forms, sorted(cm.WANT_FORMS - forms)
    print("forms:", sorted(forms))
    for lv in (cm.MIXED, cm.ROTATION):
        forms, flags = cm.coverage(lv, cm.SEED, values="edges")
        assert {"sub_wraps", "mulc_0", "mulc_max"} <= flags
        prog = cm.class_mix64(lv, cm.SEED, values="edges")[0]
        z = prog[prog["domain"] == 1]
        imms = {int(i) for i in z["imm"][np.isin(z["opcode"], (3, 7, 9))]}  # (a SubConst may subtract a clear value: zero rows, the sink)
        assert imms <= set(cm.EDGES) and len(imms) >= 6  # (of the 8 there are)
        assert set(cm.class_mix64(lv, cm.SEED, values="edges")[1]) <= set(cm.EDGES)
    assert cm.M64 in cm.EDGES and (1 << 63) in cm.EDGES and (-(1 << 32)) & cm.M64 in cm.EDGES
    # random values use all 64 bits
    assert any(w >> 63 for w in cm.class_mix64(cm.MIXED, cm.SEED)[1])
    # by level, every whole step of four Mul gates is consecutive in the preprocessing transcript; interleaved, none in the levels that
    # alternate with the Muls of the level behind them (1 and 3) and few in the others
    plain = cm.pre_runs(cm.INTERLEAVED, cm.SEED)
    inter = cm.pre_runs(cm.INTERLEAVED, cm.SEED, order="interleaved")
    assert all(broken == 0 and run > 0 for run, broken in plain.values())
    assert inter[1][0] == 0 and inter[3][0] == 0 and all(broken > run for run, broken in inter.values()), inter
    assert sorted(cm.class_mix64(cm.INTERLEAVED, cm.SEED)[0].tolist()) == sorted(cm.class_mix64(cm.INTERLEAVED, cm.SEED)[0].tolist())


def test_input_options():
    prog, wit, wc = cm.class_mix64(cm.ODD_INPUTS, cm.SEED, inputs="odd")
    assert len(wit) % 2 == 1
    with pytest.raises(ValueError):
        cm.class_mix64(cm.ODD_INPUTS, cm.SEED)  # Inputs come in pairs
    for k in (64, 65):
        prog, wit, wc = cm.class_mix64(cm.runs_spec(k), cm.SEED, inputs=("runs", k))
        z = prog["opcode"]
        at = np.flatnonzero(z == 0)
        assert len(at) == 2 * k and all(z[at[2 * j] + 1] == 0 and z[at[2 * j + 1] + 1] == 6 for j in range(k - 1))  # Input, Input, Mul, ...
    with pytest.raises(ValueError):
        cm.class_mix64(cm.runs_spec(8), cm.SEED, inputs=("runs", 9))


def test_generator_is_deterministic_and_refuses_what_it_cannot_build():
    a, b = cm.class_mix64(cm.MIXED, 3), cm.class_mix64(cm.MIXED, 3)
    assert a[0].tobytes() == b[0].tobytes() and a[1] == b[1] and a[2] == b[2]
    assert cm.class_mix64(cm.MIXED, 4)[0].tobytes() != a[0].tobytes()
    with pytest.raises(ValueError):
        cm.class_mix64([cm.L(inp=4, mul=1)], 1)  # a Mul on level 0
    with pytest.raises(ValueError):
        cm.class_mix64([cm.L(inp=4), cm.L(mul=2), cm.L(az=1)], 1)  # no gate that could write the AssertZero's zero row
    with pytest.raises(ValueError):
        cm.class_mix64([cm.L(inp=8), cm.L(subc=2), cm.L(az=2)], 1)  # six Inputs unread, and the last level writes no row
    with pytest.raises(ValueError):
        cm.class_mix64([cm.L(inp=4), cm.L(subc=4), cm.L(az=4), cm.L(add=1)], 1)  # nothing to stand behind


def test_hook_arguments():
    from reverie_amd import _lib

    lib = _lib.lib()
    prog, wit, wc = cm.class_mix64(cm.MIXED, cm.SEED)
    args = (prog.ctypes.data_as(C.c_void_p), C.c_size_t(len(prog)), C.c_size_t(wc[0]), C.c_size_t(wc[1]))
    n, why = C.c_size_t(0), C.c_int(-1)
    assert lib.rv_hook_z64_fused_levels(*args, C.c_uint32(0), None, C.c_size_t(0), C.byref(n), C.byref(why)) == 0 and n.value >= len(cm.MIXED)
    assert lib.rv_hook_z64_fused_levels(*args, C.c_uint32(0), None, C.c_size_t(0), None, C.byref(why)) == 9  # RV_E_ARG
    assert lib.rv_hook_z64_fused_levels(*args, C.c_uint32(0), None, C.c_size_t(0), C.byref(n), None) == 9
    assert lib.rv_hook_z64_fused_levels(*args, C.c_uint32(0), None, C.c_size_t(2), C.byref(n), C.byref(why)) == 9
    assert lib.rv_hook_z64_fused_levels(*args, C.c_uint32(2), None, C.c_size_t(0), C.byref(n), C.byref(why)) == 9  # unknown flag
    out = np.full((3, 4), 7, np.uint32)  # a short buffer takes the first levels and nothing behind them
    assert lib.rv_hook_z64_fused_levels(*args, C.c_uint32(0), out.ctypes.data_as(C.c_void_p), C.c_size_t(2), C.byref(n), C.byref(why)) == 0
    assert (out[2] == 7).all() and out[0, 0] == 0 and out[0, 3] == out[1, 0] == sum(cm.bounds(cm.MIXED[0]))
    grid = (C.c_uint32 * 5)()
    assert lib.rv_hook_z64_fused_grid(16, 4, 256, 1, 1, 1, None) == 9 and lib.rv_hook_z64_fused_grid(4, 4, 256, 1, 1, 1, grid) == 9
    assert lib.rv_hook_z64_fused_grid(8, 1, 256, 1, 1, 1, grid) == 0 and list(grid) == [1, 8, 8, 64, 3]
    counts = ((C.c_uint64 * 2) * 4)()
    assert lib.rv_hook_interp64_launches(None, C.c_int(0)) == 9
    assert lib.rv_hook_interp64_launches(counts, C.c_int(0)) == 0
    assert all(counts[e][m] == 0 for e in range(4) for m in range(2))  # (nothing was launched on the host)
