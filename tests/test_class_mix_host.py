"""tests/class_mix.py on the host compiler alone (rv_hook_compile_levels: no device): every spec test_gpu_level_classes.py runs must
compile, in the lazy-sum form, to exactly the class counts it asks for, level by level, and to the narrow-run plan the test was
written for -- the proof that the GPU tests aim where they say.  If a spec misses, the generator is what changes."""
import ctypes as C

import numpy as np
import pytest

import class_mix as cm

SEED = 7


def runs_of(table):
    """[(first level, end, tiny)] of the narrow runs in a level_table(); the run index must count up from 0 and hold one tiny"""
    out = []
    for l, row in enumerate(table):
        run, tiny = row[6], row[7]
        if run < 0:
            assert tiny == -1
            continue
        if run == len(out) - 1 and out[-1][1] == l:
            assert out[-1][2] == tiny
            out[-1][1] = l + 1
        else:
            assert run == len(out)
            out.append([l, l + 1, tiny])
    return [tuple(r) for r in out]


def check(levels, want_runs, seed=SEED):
    prog, wit, wc = cm.class_mix(levels, seed)
    table = cm.level_table(prog, wc)
    want = cm.class_table(levels, seed)
    assert want[:len(levels)] == [tuple(lv[:5]) for lv in levels]  # (what was asked for; then at most the sink level)
    assert len(want) <= len(levels) + 1 and all(w[:4] == (0, 0, 0, 0) for w in want[len(levels):])
    assert [row[:5] for row in table] == want
    assert not any(row[5] for row in table)  # (no Z64 gates)
    assert runs_of(table) == want_runs
    assert len(wit) == sum(lv[4] for lv in levels[:1]) - dict(levels[0][5] if len(levels[0]) > 5 else {}).get("random", 0)
    return table


@pytest.mark.parametrize("rand", [0, 1])
@pytest.mark.parametrize("cls", range(5))
@pytest.mark.parametrize("kind", ["fast", "alone", "general"])
def test_step_remainder_specs(kind, cls, rand):
    """two levels and the sink behind 300 Inputs: no run; c1 + c3 on the side of 64 the kind names"""
    specs = cm.step_specs(kind, cls, rand)
    assert [lv[1][cls] for _, lv in specs] == [n for n in (0, 1, 3, 4, 5, 7, 8, 9, 15, 16, 17, 33) if n or kind != "alone"]
    for name, levels in specs:
        table = check(levels, [])
        assert len(table) <= 3, name
        assert (table[1][1] + table[1][3] >= 64) == (kind == "general"), name
        if kind == "alone":
            assert sum(1 for c in table[1][:5] if c) == 1, name


def test_slot_rotation_specs():
    for name, levels in cm.SLOT_SPECS:
        table = check(levels, [])
        assert 1 <= sum(table[1][:5]) <= 5 and sum(1 for c in table[1][:5] if c) == 3, name


@pytest.mark.parametrize("c1,c3", cm.GENERAL_SWITCH)
def test_general_switch_specs(c1, c3):
    for rand in (0, 1):
        table = check(cm.switch_own(c1, c3, rand), [])
        assert sum(table[1][:5]) == 300 and (table[1][1], table[1][3]) == (c1, c3)
    # in a run: eight levels wider than 32 gates are one class-loop piece (not lean: multi-base gates), the sink of 21 a per-gate one
    table = check(cm.switch_in_run(c1, c3), [(1, 9, 0), (9, 10, 1)])
    assert (table[5][1], table[5][3]) == (c1, c3) and all(32 < sum(row[:5]) <= 256 for row in table[1:9])


def test_vclr_edge_specs():
    """16 levels in narrow runs, and 17: MODE_PROVE_V's limit (csrc/api.hip: vclr_ok)"""
    for n in (16, 17):
        table = check(cm.VCLR_SPECS[n], [(1, n + 1, 1)])
        assert len(table) == n + 1


@pytest.mark.parametrize("name", sorted(cm.RUN_SPECS))
def test_run_plan_specs(name):
    levels, want_runs = cm.RUN_SPECS[name]
    table = check(levels, want_runs)
    width = [sum(row[:5]) for row in table]
    in_run = [row[6] >= 0 for row in table]
    l = 0
    while l < len(table):  # every class is present somewhere in each narrow stretch (a lean one holds no multi-base gate)
        if not in_run[l]:
            l += 1
            continue
        e = l
        while e < len(table) and in_run[e]:
            e += 1
        for k in range(5):
            assert any(table[i][k] for i in range(l, e)) or (name in ("lean", "not-lean") and k in (1, 3)), (name, l, e, k)
        l = e
    if name in ("lean", "not-lean"):  # the same stretch, with one multi-base gate in one of its levels
        assert sum(row[1] + row[3] for row in table[1:9]) == (name == "not-lean")
        assert [sum(r[:5]) for r in table] == [sum(r[:5]) for r in check(cm.RUN_SPECS["lean"][0], cm.RUN_SPECS["lean"][1])]
    if name == "7x33-8x33-8x32":
        assert width[1:8] == [33] * 7 and width[9:17] == [33] * 8 and width[18:26] == [32] * 8
    if name in ("256", "257"):
        assert width[2] == int(name)
    if name == "window":
        # the 1024-record window is refilled in front of a level that does not start where a window would end
        assert width[1:10] == cm.WINDOW_WIDTHS[:9]
        lo, win_hi, refills = 0, 0, []
        for l in range(1, 12):
            if lo + width[l] > win_hi:
                refills.append(lo)
                win_hi = lo + 1024
            lo += width[l]
        assert len(refills) >= 3 and all(r % 1024 for r in refills[1:])
    if name == "1025":
        assert want_runs[0][1] - want_runs[0][0] == 1025 and min(width[1:]) > 32


def test_grid_and_batch_specs():
    for name, levels in cm.GRID_SPECS.items():
        table = check(levels, [])
        assert all(c > 0 for c in table[1][:5]) or name == "prefetch-no-next"
    assert sum(check(cm.GRID_SPECS["cap-fast"], [])[1][:5]) == 70000  # more than the 65 536 gates 4 096 workgroups take in one pass
    assert sum(check(cm.GRID_SPECS["cap-general"], [])[1][:5]) == 70000
    t = check(cm.GRID_SPECS["prefetch-tiny-next"], [])
    assert [sum(r[:5]) for r in t[1:3]] == [20000, 1]
    assert len(check(cm.GRID_SPECS["prefetch-no-next"], [])) == 2  # (no sink: the level with the class loops is the last launch)
    check(cm.BATCH_OWN, [])
    assert [c % 4 for c in cm.BATCH_OWN[1]] == [1, 2, 3, 1, 3]
    check(cm.BATCH_RUN, [(1, 8, 1), (8, 17, 0), (17, 18, 1)])


def test_generator_is_deterministic_and_refuses_what_it_cannot_build():
    a = cm.class_mix([cm.wide0(), (5, 6, 7, 9, 3)], 3)
    b = cm.class_mix([cm.wide0(), (5, 6, 7, 9, 3)], 3)
    assert a[0].tobytes() == b[0].tobytes() and a[1] == b[1] and a[2] == b[2]
    assert cm.class_mix([cm.wide0(), (5, 6, 7, 9, 3)], 4)[0].tobytes() != a[0].tobytes()
    with pytest.raises(ValueError):
        cm.class_mix([(1, 0, 0, 0, 8)], 1)  # a one-base Mul on level 0
    with pytest.raises(ValueError):
        cm.class_mix([(0, 0, 0, 0, 8), (0, 0, 0, 0, 3), (1, 0, 0, 0, 0)], 1)  # nothing to stand behind: level 1 writes no row
    with pytest.raises(ValueError):
        cm.class_mix([(0, 0, 0, 0, 3), (0, 0, 0, 1, 0)], 1)  # a sum of up to 6 distinct rows out of 3


def test_level_hook_arguments_and_plain_form():
    from reverie_amd import _lib

    L = _lib.lib()
    prog, wit, wc = cm.class_mix(cm.RUN_SPECS["merge"][0], SEED)
    args = (prog.ctypes.data_as(C.c_void_p), C.c_size_t(len(prog)), C.c_size_t(wc[0]), C.c_size_t(wc[1]))
    n = C.c_size_t(0)
    assert L.rv_hook_compile_levels(*args, C.c_uint32(1), None, C.c_size_t(0), C.byref(n)) == 0 and n.value == 11
    assert L.rv_hook_compile_levels(*args, C.c_uint32(1), None, C.c_size_t(0), None) == 9  # RV_E_ARG
    assert L.rv_hook_compile_levels(*args, C.c_uint32(1), None, C.c_size_t(4), C.byref(n)) == 9
    assert L.rv_hook_compile_levels(*args, C.c_uint32(2), None, C.c_size_t(0), C.byref(n)) == 9  # unknown flag
    # a short buffer takes the first levels and nothing behind them
    out = np.full((5, 10), -7, np.int32)
    assert L.rv_hook_compile_levels(*args, C.c_uint32(1), out.ctypes.data_as(C.c_void_p), C.c_size_t(4), C.byref(n)) == 0 and n.value == 11
    full = cm.level_table(prog, wc)
    assert (out[4] == -7).all() and [int(x) for x in out[0, :6]] == [0, 0, 0, 0, 0, 300]
    assert [tuple(int(x) for x in r[6:9]) for r in out[:4]] == [row[5:8] for row in full[:4]] and (out[:4, 9] == -1).all()
    # the plain form materialises every sum: other classes, the same program (the specs are for the lazy-sum form)
    plain = cm.level_table(prog, wc, whole_prover=False)
    assert [r[:5] for r in plain] != [r[:5] for r in full]
    assert sum(r[0] + r[1] for r in plain) == sum(r[0] + r[1] for r in full)  # (every Mul is a gate either way)
    counts = ((C.c_uint64 * 4) * 11)()
    assert L.rv_hook_interp_launches(None, C.c_int(0)) == 9
    assert L.rv_hook_interp_launches(counts, C.c_int(0)) == 0
