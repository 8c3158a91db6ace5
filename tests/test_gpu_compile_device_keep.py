"""RV_COMPILE_KEEP_WIRES in the device compiler (RV_COMPILE_DEVICE_KEEP_WIRES, csrc/compile_dev.hip): the host compiler's Compiled
field by field, wire_forms and wire_ssa64 included, in every scope the device compiler has (GF(2), with Z64, with B2A) and both
gate-stream forms; what the device path still hands back keeps the host's status; without the bit nothing changes.  Every case
compares against the host compiler (rv_hook_compile_compare_device), never against the device path itself."""
import numpy as np
import pytest

import lazy_corpus
from reverie_amd.ops import B2A, GF2, OP_DTYPE, SizeHint, Z64, program
from test_gpu_compile_device_b2a import gen_b2a, wide_program
from test_gpu_compile_device_z64 import _no_times, compare, gen_mixed, lazy_forms_pay, programs

pytestmark = pytest.mark.gpu

WP, KEEP, DEV, DEVZ, DEVB, DK = 1, 2, 4, 12, 44, 128


def k1_final_keep(prog, wc, monkeypatch):
    """True when the K = 1 compile with RV_COMPILE_KEEP_WIRES is the host compiler's final answer (compile.h: lazy_forms_pay of its
    level and gate counts; the kept final sums are gates of that compile)"""
    import reverie_amd

    with monkeypatch.context() as m:
        m.setenv("RV_LAZY_K", "1")
        c = reverie_amd.Circuit(prog, wc, keep_wires=True)
    info = c.info
    c.close()
    return not lazy_forms_pay(info["levels"], info["gf2_inputs"] + info["gf2_muls"] + info["gf2_asserts"] + info["gf2_linear"])


def check_both_forms(prog, wc, scope, monkeypatch, what="", plain_on_device=None):
    """the lazy-sum form: taken; the plain form: taken exactly when the K = 1 compile is final (plain_on_device: what that has to
    be for this program); no difference from the host compiler's RV_COMPILE_KEEP_WIRES circuit either way"""
    assert compare(prog, wc, scope | WP | KEEP | DK) == (0, 1, 0), (what, "lazy")
    final = k1_final_keep(prog, wc, monkeypatch)
    if plain_on_device is not None:
        assert final == plain_on_device, (what, final)
    assert compare(prog, wc, scope | KEEP | DK) == (0, int(final), 0), (what, "plain", final)


def inputs(n, first=0):
    return [GF2.Input(first + i) for i in range(n)]


def gf2_hand_programs():
    """name -> (ops, wire counts): GF(2) programs, every one a few levels deep (final in the plain form)"""
    sum3 = inputs(4) + [GF2.Add(4, 0, 1), GF2.Add(5, 4, 2)]  # wire 4: a ^ b (read once, and final), wire 5: a ^ b ^ c
    out = {
        # the last op is read by nothing: without the read after the program the sum is dropped and wire 2 reads 0
        "unread_last_add": (inputs(2) + [GF2.Add(2, 0, 1)], (0, 3)),
        # only the last writer's value counts; the two earlier sums are read by nothing and still dropped
        "overwritten_three_times": (inputs(3) + [GF2.Add(3, 0, 1), GF2.Add(3, 0, 2), GF2.Add(3, 1, 2)], (0, 4)),
        "overwritten_by_a_constant": (inputs(2) + [GF2.Add(2, 0, 1), GF2.Const(2, 1)], (0, 3)),
        # final values without a row of their own: constants, aliases of an input row (with and without the constant), MulConst by
        # 0 and by 1, x ^ x, an alias plus its row (the constant 1)
        "constants_and_aliases": ([GF2.Const(0, 1), GF2.Const(1, 0), GF2.Input(2), GF2.AddConst(3, 2, 1), GF2.AddConst(4, 2, 0), GF2.MulConst(5, 2, 0),
                                   GF2.MulConst(6, 2, 1), GF2.Add(7, 2, 2), GF2.Add(8, 3, 2), GF2.SubConst(9, 3, 1)], (0, 10)),
        # a sum of RV_LIN_K rows as a final value (symbolic in the lazy-sum form: all three slots used), and one of RV_LIN_K + 1
        "sum_of_k_rows": (sum3, (0, 6)),
        "sum_of_k_plus_1_rows": (sum3 + [GF2.Add(6, 5, 3)], (0, 7)),
        "sum_of_k_rows_with_constant": (sum3 + [GF2.AddConst(5, 5, 1)], (0, 6)),
        # two wires assigned the same row: two reads of the sum by the aliases, each alias read once after the program
        "two_wires_one_row": (inputs(2) + [GF2.Add(2, 0, 1), GF2.AddConst(3, 2, 0), GF2.AddConst(4, 2, 1)], (0, 5)),
        "mul_results_and_asserts": (inputs(3) + [GF2.Mul(3, 0, 1), GF2.Add(4, 3, 2), GF2.AssertZero(4), GF2.Mul(3, 4, 4), GF2.Random(5), GF2.Add(6, 5, 3)], (0, 7)),
        # no wire is ever written
        "asserts_only": ([GF2.AssertZero(0), GF2.AssertZero(3)], (0, 5)),
    }
    # a wire never written, gf2_wires larger than any wire used, around one workgroup of the per-wire kernels
    for w in (1, 255, 256, 257):
        out["wires_%d_one_input" % w] = ([GF2.Input(0)], (0, w))
        out["wires_%d_last_wire" % w] = (inputs(2) + [GF2.Add(w - 1, 0, 1)] if w > 2 else [GF2.Const(w - 1, 1)], (0, w))
    out["wires_257_holes"] = (inputs(2) + [GF2.Add(k, 0, 1) for k in (2, 100, 254, 255, 256)] + [GF2.AddConst(255, 255, 1)], (0, 257))
    out["wires_1000_three_used"] = (inputs(2) + [GF2.Mul(2, 0, 1)], (0, 1000))
    return out


def flip_programs():
    """The lazy rule's flip.  Wire 5 = a ^ b ^ c, a sum of 3 rows read by exactly two ops.  `final`: it is also its wire's final
    value, so f = 3 and 3 x 2 > 3 + 1: materialised.  `not_final`: the wire is overwritten afterwards, f = 2 and 2 x 2 <= 3 + 1: it
    stays symbolic.  (Wire 4 = a ^ b is read once and final either way: f = 2, symbolic.)"""
    body = inputs(4) + [GF2.Add(4, 0, 1), GF2.Add(5, 4, 2), GF2.Mul(6, 5, 3), GF2.Mul(7, 5, 0)]
    return program(body), program(body + [GF2.Const(5, 0)]), (0, 8)


def mixed_hand_programs():
    """name -> (ops, wire counts, scope): the Z64 side's cases, and B2A"""
    src = inputs(64)
    return {
        "z64_never_written": ([Z64.Input(0), Z64.AddConst(2, 0, 1), GF2.Input(0)], (5, 2), DEVZ),
        "z64_overwritten": ([Z64.Input(0), Z64.Input(1), Z64.Add(2, 0, 1), Z64.Mul(2, 0, 1), Z64.Sub(2, 2, 0), Z64.Input(0), GF2.Input(0)], (3, 1), DEVZ),
        "z64_const_only": ([Z64.Const(0, 7), Z64.Const(3, 0), Z64.Const(0, 9), GF2.Const(1, 1)], (4, 2), DEVZ),
        "z64_asserts_only": ([Z64.AssertZero(1), GF2.Input(0), GF2.Input(1), GF2.Add(2, 0, 1)], (3, 3), DEVZ),
        "no_z64_wires": (inputs(3) + [GF2.Add(3, 0, 1), GF2.Mul(4, 3, 2), GF2.Add(5, 4, 3)], (0, 6), DEVZ),
        "z64_wires_but_gf2_ops_only": (inputs(3) + [GF2.Add(3, 0, 1), GF2.Mul(4, 3, 2), GF2.Add(5, 4, 3)], (7, 6), DEVZ),
        "z64_wires_but_gf2_ops_only_gf2_scope": (inputs(3) + [GF2.Add(3, 0, 1), GF2.Mul(4, 3, 2), GF2.Add(5, 4, 3)], (7, 6), DEV),
        "no_gf2_wires": ([Z64.Input(0), Z64.Input(1), Z64.Mul(2, 0, 1), Z64.AddConst(0, 2, 5), Z64.AssertZero(3)], (5, 0), DEVZ),
        "gf2_wires_but_z64_ops_only": ([Z64.Input(0), Z64.Input(1), Z64.Mul(2, 0, 1), Z64.AddConst(0, 2, 5)], (3, 300), DEVZ),
        "sizehint_that_grows_nothing": ([SizeHint(3, 4), GF2.Input(0), Z64.Input(0), SizeHint(0, 0), GF2.AddConst(3, 0, 1), Z64.MulConst(2, 0, 3)], (3, 4), DEVZ),
        "sizehints_only_beside_gf2": ([SizeHint(2, 3)] + inputs(2) + [GF2.Add(2, 0, 1)], (2, 3), DEVZ),
        "wires_256_both": ([Z64.Input(255), GF2.Input(255), Z64.AddConst(0, 255, 1), GF2.AddConst(0, 255, 1)], (256, 256), DEVZ),
        "wires_257_both": ([Z64.Input(256), GF2.Input(256), Z64.AddConst(0, 256, 1), GF2.AddConst(0, 256, 1)], (257, 257), DEVZ),
        # B2A: its 64 source wires are final values, its result is the final value of a Z64 wire
        "b2a_sources_final": (src + [B2A(0, 0)], (1, 64), DEVB),
        "b2a_last_writer": ([Z64.Input(1), Z64.Const(0, 3)] + src + [B2A(0, 0), Z64.Add(2, 0, 1)], (4, 64), DEVB),
        "b2a_destination_overwritten": (src + [B2A(0, 0), Z64.AddConst(1, 0, 1), Z64.Const(0, 7)], (2, 64), DEVB),
        "b2a_sources_overwritten": (src + [B2A(0, 0)] + [GF2.Add(k, k, (k + 1) % 64) for k in range(0, 64, 3)] + [B2A(1, 0)], (2, 64), DEVB),
        "b2a_sources_never_written": ([B2A(1, 3), GF2.Input(70)], (2, 71), DEVB),
        "b2a_sources_are_sums": (inputs(8, 64) + [GF2.Add(k, 64 + k % 8, 64 + (k + 1) % 8) for k in range(64)] + [B2A(0, 0)], (1, 72), DEVB),
    }


# ---- 1. hand-written programs ----
@pytest.mark.parametrize("name", sorted(gf2_hand_programs()))
def test_gf2_hand_programs(monkeypatch, name):
    ops, wc = gf2_hand_programs()[name]
    for scope in (DEV, DEVZ, DEVB):
        check_both_forms(program(ops), wc, scope, monkeypatch, (name, scope), plain_on_device=True)


def _info(prog, wc, **kw):
    import reverie_amd

    c = reverie_amd.Circuit(prog, wc, keep_wires=True, **kw)
    info, on_dev = c.info, c.compiled_on_device
    c.close()
    return info, on_dev


def test_lazy_rule_flip(monkeypatch):
    final, not_final, wc = flip_programs()
    for prog in (final, not_final):
        check_both_forms(prog, wc, DEV, monkeypatch, plain_on_device=True)
    kw = {"whole_prover": True, "device_compile": True, "device_keep_wires": True}
    a, on_a = _info(final, wc, **kw)
    b, on_b = _info(not_final, wc, **kw)
    assert on_a and on_b
    # the materialised sum is one more linear gate, one more row written and one level more (the two Mul gates read its row)
    assert a["gf2_linear"] == b["gf2_linear"] + 1 and a["gf2_rows_written"] == 1 and b["gf2_rows_written"] == 0
    assert a["levels"] == 3 and b["levels"] == 2
    # ... and the host compiler says the same of both
    assert _info(final, wc, whole_prover=True)[0]["gf2_rows_written"] == 1 and _info(not_final, wc, whole_prover=True)[0]["gf2_rows_written"] == 0


def test_unread_sums(monkeypatch):
    """the final sum is kept, the overwritten ones are dropped: one linear gate in either program, in either form"""
    for name in ("unread_last_add", "overwritten_three_times"):
        ops, wc = gf2_hand_programs()[name]
        for wp in (False, True):
            info, on_dev = _info(program(ops), wc, whole_prover=wp, device_compile=True, device_keep_wires=True)
            # (in the lazy-sum form a two-row sum read once stays symbolic: no gate at all)
            assert on_dev and info["gf2_rows_written"] == (0 if wp else 1), (name, wp)
            assert _no_times(info) == _no_times(_info(program(ops), wc, whole_prover=wp)[0]), (name, wp)


@pytest.mark.parametrize("name", sorted(mixed_hand_programs()))
def test_mixed_hand_programs(monkeypatch, name):
    ops, wc, scope = mixed_hand_programs()[name]
    check_both_forms(program(ops), wc, scope, monkeypatch, name, plain_on_device=None if scope == DEVB else True)
    if scope != DEVB and scope != DEV:  # (a wider scope takes what a narrower one does)
        check_both_forms(program(ops), wc, DEVB, monkeypatch, name)


def test_wide_b2a_program_in_the_plain_form(monkeypatch):
    """adders side by side: the one kind of B2A program that is final at K = 1, so the plain form with B2A is compared too"""
    n_b2a = 128
    while not k1_final_keep(*wide_program(n_b2a), monkeypatch):  # (wider when the rule says otherwise)
        n_b2a *= 2
        assert n_b2a <= 1024
    prog, wc = wide_program(n_b2a)
    check_both_forms(prog, wc, DEVB, monkeypatch, plain_on_device=True)


# ---- 2. random programs ----
def _random_cases(scope):
    """(name, program, wire counts): 50 to 400 ops, twelve and more per scope"""
    out = []
    if scope == DEV:
        small = [(p, wc) for p, _, wc in lazy_corpus.random_programs() if 50 <= len(p) <= 400]
        out += [("corpus%d" % k, p, wc) for k, (p, wc) in enumerate(small[:8])]
        for seed in range(8):
            rng = np.random.default_rng(0x6EE900 + seed)
            n, w = int(rng.integers(50, 401)), int(rng.choice([3, 12, 65, 255, 256, 257, 600]))
            out.append(("gf2_%d" % seed, gen_mixed(rng, n, 0, w, 0.0, hints=False)[0], (int(rng.choice([0, 4])), w)))
        crafted, _, crafted_wc = lazy_corpus.crafted_program()
        out.append(("crafted", crafted, crafted_wc))
    elif scope == DEVZ:
        out += [(name, p, wc) for name, p, wc, _ in programs() if 50 <= len(p) <= 400]
        for seed in range(8):
            rng = np.random.default_rng(0x6EE964 + seed)
            n, w64, w2 = int(rng.integers(50, 401)), int(rng.choice([3, 12, 65, 257])), int(rng.choice([3, 12, 65, 257]))
            out.append(("mixed_%d" % seed, gen_mixed(rng, n, w64, w2, float(rng.choice([0.1, 0.5, 0.9])))[0], (w64, w2)))
    else:
        for seed in range(12):
            rng = np.random.default_rng(0x6EEB2A + seed)
            n, w64, w2 = int(rng.integers(50, 401)), int(rng.choice([3, 12, 65])), int(rng.choice([64, 65, 100, 257]))
            prog, _, _, wc = gen_b2a(rng, n, w64, w2, float(rng.choice([0.1, 0.5, 0.9])))
            out.append(("b2a_%d" % seed, prog, wc))
    return out


@pytest.mark.parametrize("scope", [DEV, DEVZ, DEVB])
def test_random_programs(monkeypatch, scope):
    cases = _random_cases(scope)
    assert len(cases) >= 12 and all(50 <= len(p) <= 400 + 7 for _, p, _ in cases)  # (gen_b2a adds its B2A ops to the count asked for)
    n_plain = 0
    for name, prog, wc in cases:
        assert compare(prog, wc, scope | WP | KEEP | DK) == (0, 1, 0), (name, "lazy")
        rc, path, diff = compare(prog, wc, scope | KEEP | DK)
        assert (rc, diff) == (0, 0) and path == int(k1_final_keep(prog, wc, monkeypatch)), (name, "plain", rc, path, diff)
        n_plain += path
    assert n_plain or scope == DEVB  # (one adder is some 190 levels deep: no small program with a B2A is final in the plain form)


# ---- 3. scope ----
def test_what_the_device_still_hands_back():
    grows2 = program(inputs(2) + [SizeHint(0, 9), GF2.Add(8, 0, 1)])
    grows64 = program([Z64.Input(0), SizeHint(9, 0), Z64.AddConst(8, 0, 1), GF2.Input(0)])
    oob = program(inputs(2) + [GF2.Add(3, 0, 1)])
    oob64 = program([Z64.Input(0), Z64.Add(1, 0, 3), GF2.Input(0)])
    reserved = program(inputs(2) + [GF2.Add(2, 0, 1)])
    reserved["reserved"][2] = 1
    for name, prog, wc, want in (("grows_gf2", grows2, (0, 3), 0), ("grows_z64", grows64, (1, 1), 0), ("gf2_oob", oob, (0, 3), 3),
                                 ("z64_oob", oob64, (3, 1), 3), ("reserved", reserved, (0, 3), 5)):
        for scope in (DEVZ, DEVB):
            for wp in (0, WP):
                assert compare(prog, wc, scope | wp | KEEP | DK) == (want, 0, 0), (name, scope, wp)
    # the same programs without their fault are taken
    assert compare(program(inputs(2) + [SizeHint(0, 9), GF2.Add(8, 0, 1)]), (0, 9), DEVZ | KEEP | DK) == (0, 1, 0)
    assert compare(oob, (0, 4), DEVZ | KEEP | DK) == (0, 1, 0)
    # an empty program is the host compiler's
    assert compare(np.zeros(0, OP_DTYPE), (2, 2), DEVZ | KEEP | DK) == (0, 0, 0)


def test_without_the_bit_nothing_changes(monkeypatch):
    import reverie_amd

    prog, wc = program(inputs(2) + [GF2.Add(2, 0, 1)]), (0, 3)
    mixed = gen_mixed(np.random.default_rng(3), 300, 20, 20, 0.5)[0]
    for p, w in ((prog, wc), (mixed, (20, 20))):
        for scope in (DEV, DEVZ, DEVB):
            for wp in (0, WP):
                assert compare(p, w, scope | wp | KEEP) == (0, 0, 0)  # RV_COMPILE_KEEP_WIRES alone stays the host compiler's
    for scope in (DEV, DEVZ, DEVB):
        for wp in (0, WP):
            assert compare(prog, wc, scope | wp | KEEP | DK) == (0, 1, 0)
    c = reverie_amd.Circuit(prog, wc, keep_wires=True, device_compile=True)
    assert not c.compiled_on_device
    c.close()
    c = reverie_amd.Circuit(prog, wc, keep_wires=True, device_compile=True, device_keep_wires=True)
    assert c.compiled_on_device and c.evaluate([1, 0]).gf2.tolist() == [1, 0, 1]
    c.close()
    # RV_LAZY_K in the environment stays a fallback under the new bit too
    monkeypatch.setenv("RV_LAZY_K", "2")
    assert compare(prog, wc, DEV | KEEP | DK) == (0, 0, 0)
