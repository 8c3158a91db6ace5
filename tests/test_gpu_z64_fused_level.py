"""k_z64_fused (csrc/aes.hip) launch by launch against tests/z64f_ref.py, every buffer whole and bit for bit.

rv_hook_z64_fused_run calls the production launcher unchanged, once per level, on records and buffers the test supplies, so what whole
proofs fix is free here: first_block (the counter window, up to the last legal counter 2^24 - 1 and across every carry into counter bits
16..23), the quad-group range (qg0, qgn), the transcript offsets, and whether a wavefront's four Muls are consecutive in the
preprocessing stream.  The reference is tied to the oracle without a device by tests/test_z64f_ref_host.py; the cases and their
independence checks are tests/z64f_cases.py.  Every output starts as 0xA5 bytes (the error word as 0) and must still be 0xA5 wherever
the reference defines no word: a dropped gate shows as an untouched word, a doubled or misplaced one as a wrong word.

Widths: R = 32 and 96 run blocks of QW = 8 quad words (one and three quad groups), R = 64, 128 and 256 blocks of 16 (one, two, four)."""
import ctypes as C

import numpy as np
import pytest

import b3_ref
import class_mix64 as cm
import z64f_cases as zc
import z64f_ref as zr

pytestmark = pytest.mark.gpu

WIDTHS = [32, 96, 64, 128, 256]
MODES = ["prove", "verify"]
E_UNSUPPORTED, E_ARG = 8, 9
FILL32 = 0xA5A5A5A5


def _seeds(R):
    return np.random.default_rng(6400 + R).integers(0, 256, (R, 16), dtype=np.uint8)


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


@pytest.fixture(scope="module")
def hook(oracle):
    import reverie_amd
    from reverie_amd import _lib

    ctx = reverie_amd.Context.default()  # raises loudly if the HIP library or the GPU is missing

    def call(case, seeds, omit, first_block, qg0, qgn, sup=None, key_path=0, sup_r=None, levels=None, gates=None):
        R = len(seeds)
        bufs = {"wmask": np.full((case.n_ssa, R * 8), zr.FILL), "masks": np.full((case.n_rows, R * 8), zr.FILL), "v": np.full(case.n_ssa, zr.FILL),
                "wcorr": np.full((case.n_ssa, R), zr.FILL), "on": np.full((R, case.on_words), zr.FILL), "pre": np.full((R, case.pre_words), zr.FILL),
                "err": np.zeros(1, np.int32)}
        gates = case.gates if gates is None else gates
        levels = case.levels if levels is None else levels
        keep = [np.ascontiguousarray(seeds), None if omit is None else np.ascontiguousarray(omit), np.ascontiguousarray(gates), np.ascontiguousarray(levels)]
        a = _lib.Z64FRunArgs()
        a.seeds, a.omit, a.R, a.key_path, a.first_block, a.qg0, a.qgn = _p(keep[0]).value, _p(keep[1]) and _p(keep[1]).value, R, key_path, first_block, qg0, qgn
        a.gates, a.n_gates, a.levels, a.n_levels = _p(keep[2]).value, len(gates), _p(keep[3]).value, len(levels)
        a.runs, a.n_runs, a.on_words, a.pre_words = _p(case.runs).value, len(case.runs), case.on_words, case.pre_words
        a.wit, a.n_wit = _p(case.wit).value if len(case.wit) else None, len(case.wit)
        if sup is not None:
            sup = [np.ascontiguousarray(s, np.uint64) for s in sup]
            a.sup_in, a.sup_corr, a.sup_rec = (_p(s).value for s in sup)
            a.sup_r = sup[0].shape[1] if sup_r is None else sup_r
        a.n_in, a.n_corr, a.n_rec, a.n_ssa, a.n_mask_rows = case.n_in, case.n_corr, case.n_rec, case.n_ssa, case.n_rows
        for k in ("wmask", "masks", "v", "wcorr", "on", "pre", "err"):
            setattr(a, k, _p(bufs[k]).value)
        rc = _lib.lib().rv_hook_z64_fused_run(ctx.handle, C.byref(a))
        return rc, bufs

    return call


def _untouched(bufs):
    return all((b == zr.FILL).all() for k, b in bufs.items() if k != "err") and bufs["err"][0] == 0


def _compare(got, ref, where):
    """every buffer of the hook call against the reference's stored view; the other mode's value buffer must not have been touched"""
    want = ref.stored()
    other = "v" if ref.verify else "wcorr"
    assert (got[other] == zr.FILL).all(), f"{where}: {other} was written"
    for name, w in want.items():
        g = got[name].reshape(w.shape)
        if not np.array_equal(g, w):
            pytest.fail(f"{where}: {zr.first_diff(name, g, w)}")


def _run_both(hook, case, R, mode, first_block, qg0=0, qgn=None, omit_kind="mix", honest=True, key_path=0):
    """one hook call and its reference -> (got, ref, omit)"""
    seeds = _seeds(R)
    n_qg = (R // 4) // zr.qw_of(R // 4)
    qgn = n_qg - qg0 if qgn is None else qgn
    omit = sup = None
    if mode == "verify":
        omit = zc.omits(R, omit_kind)
        if honest:
            sup = zc.honest_sup(case, zc.run_ref(case, seeds, None, first_block), omit)
        else:
            rng = np.random.default_rng(R)
            sup = [rng.integers(0, 1 << 63, (max(n, 1), R), dtype=np.uint64) * 2 + 1 for n in (case.n_in, case.n_corr, case.n_rec)]
    ref = zc.run_ref(case, seeds, omit, first_block, qg0, qgn, sup)
    rc, got = hook(case, seeds, omit, first_block, qg0, qgn, sup, key_path)
    where = f"{case.name}, R = {R}, {mode}, first_block {first_block} = 0x{first_block:06x}, quad groups [{qg0}, {qg0 + qgn})" + (f", omit {omit_kind}" if omit is not None else "")
    assert rc == 0, f"{where}: error {rc}"
    _compare(got, ref, where)
    return got, ref, omit


# ---------------------------------------------------------------- counters
def _windows(n):
    """first_block values for a case whose blocks are 0 .. n: the start, the carry of counter byte 15 into byte 14, bytes 14 and 15 into
    13, every step from 2^k - 1 to 2^k for the counter bits 16..23 (block 0 -- an Input's and the first Mul's -- before it, the rest
    behind), and the window whose last Mul sits on the last legal counter 2^24 - 1"""
    return [0, 250, 65530] + [(1 << k) - 1 for k in range(16, 24)] + [zc.MAX_CTR - 1 - n]


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("R", WIDTHS)
def test_counter_windows(hook, R, mode):
    """a Mul level of 9 gates beside an Input level (one Input on an odd row whose cipher block is also the first Mul's) at every window"""
    case = zc.counters(9)
    for fb in _windows(9):
        got, ref, _ = _run_both(hook, case, R, mode, fb, honest=False)
        assert fb + case.last_block() < zc.MAX_CTR


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("n_mul", [4, 12])
def test_last_counter_and_one_past(hook, n_mul, mode):
    """Mul levels of 4 and 12 gates ending on counter 2^24 - 1; one block further the call is refused with nothing written"""
    case = zc.counters(n_mul)
    for R in (32, 256):
        _run_both(hook, case, R, mode, zc.MAX_CTR - 1 - n_mul, key_path=1)
        omit = zc.omits(R, "mix") if mode == "verify" else None
        sup = [np.zeros((max(n, 1), R), np.uint64) for n in (case.n_in, case.n_corr, case.n_rec)] if mode == "verify" else None
        rc, bufs = hook(case, _seeds(R), omit, zc.MAX_CTR - n_mul, 0, 1, sup)
        assert rc == E_UNSUPPORTED and _untouched(bufs)


# ---------------------------------------------------------------- quad-group ranges
def _ranges(n):
    return sorted({(0, n), (1, n - 1), (0, 1), (1, 1), (n - 1, 1)} - {(1, 0)}) if n > 1 else [(0, 1)]


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("R", WIDTHS)
def test_quad_group_ranges(hook, R, mode):
    """(0, n), (1, n - 1), (0, 1), a middle (1, 1) and the last group alone: rows, corrections and transcript words of the other groups
    stay 0xA5 (the Input rows excepted, which the generator writes for every group), v is written only with quad word 0 in the range"""
    n_qg = (R // 4) // zr.qw_of(R // 4)
    per = 4 * zr.qw_of(R // 4)
    for case in (zc.operands(True), zc.placement(1, 0, "run")):
        for qg0, qgn in _ranges(n_qg):
            got, ref, _ = _run_both(hook, case, R, mode, 3, qg0, qgn)
            out = np.ones(R, bool)
            out[qg0 * per:(qg0 + qgn) * per] = False
            assert (got["on"][out] == zr.FILL).all() and (got["pre"][out] == zr.FILL).all() and (got["wmask"].reshape(-1, R, 8)[:, out] == zr.FILL).all()
            if mode == "prove":
                assert (got["v"] == zr.FILL).all() == (qg0 != 0)
                assert got["err"][0] == (zr.E_WITNESS_INVALID if qg0 == 0 else 0)  # (both cases assert a non-zero value)
            else:
                assert (got["wcorr"][:, out] == zr.FILL).all()


# ---------------------------------------------------------------- level shapes
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("R", WIDTHS)
def test_level_shapes(hook, R, mode):
    """Mul levels of 1, JW - 1, JW, JW + 1, 8 JW - 1, 8 JW + 1 and 100 gates (several chunks per quad group), bare, with linear gates and
    with all three classes; an other-only and a linear-only level"""
    case = zc.shapes(64 // zr.qw_of(R // 4))
    _run_both(hook, case, R, mode, 65536 - 40, key_path=1 if R in (64, 256) else 0)


# ---------------------------------------------------------------- transcript placement
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("R", WIDTHS)
def test_transcript_placement(hook, R, mode):
    """on_words odd and even with eo odd and even (both branches of the eight-word store, 16-byte stores on 8-byte boundaries); ep
    consecutive over a wavefront's four gates, with a gap, and in a wavefront with gates missing; QW 8 (R = 32, 96) never takes pre_run"""
    for pad in (0, 1):
        for tail in (0, 1):
            for lay in ("run", "gap"):
                _run_both(hook, zc.placement(pad, tail, lay), R, mode, 0, omit_kind="mix" if pad else "none")


# ---------------------------------------------------------------- operands, values, omits
@pytest.mark.parametrize("R", WIDTHS)
def test_operands_and_values_prover(hook, R):
    got, ref, _ = _run_both(hook, zc.operands(False), R, "prove", 1)
    assert got["err"][0] == 0
    got, ref, _ = _run_both(hook, zc.operands(True), R, "prove", 1)
    assert got["err"][0] == zr.E_WITNESS_INVALID


@pytest.mark.parametrize("omit_kind", ["none", "mix"])
@pytest.mark.parametrize("R", WIDTHS)
def test_operands_values_and_omits_verifier(hook, R, omit_kind):
    """nobody opened; a mix with every player, a quad word opened whole and opened neighbours on both sides of every group edge.  With
    the values an honest proof carries, a true AssertZero raises nothing and a false one the zero-check bit, for opened repetitions
    only; with other values (taken by ordinal all the same) the buffers still follow the reference"""
    got, ref, omit = _run_both(hook, zc.operands(False), R, "verify", 1, omit_kind=omit_kind)
    assert got["err"][0] == 0
    # the hidden player's masks are zero: every row a Mul wrote, natural order
    P = zr.stored_index(R // 4)
    case = zc.operands(False)
    rows = case.gates["m"][case.gates["op"] == zr.MUL] + 1
    nat = got["masks"][:, P].reshape(-1, R, 8)[rows]
    opened = np.flatnonzero(omit < 8)
    assert (nat[:, opened, omit[opened]] == 0).all() and (omit_kind == "none" or (nat[:, opened, (omit[opened] + 1) % 8] != 0).all())
    got, ref, _ = _run_both(hook, zc.operands(True), R, "verify", 1, omit_kind=omit_kind)
    assert got["err"][0] == (zr.DEV_ZERO_CHECK if omit_kind == "mix" else 0)
    _run_both(hook, zc.operands(True), R, "verify", 1, omit_kind=omit_kind, honest=False)


def test_supplied_rows_of_64(hook):
    """sup_r = 64 under rows of 128 repetitions (the opened ones among the first 64, as the verifier's split schedule has them)"""
    R, case = 128, zc.operands(False)
    seeds = _seeds(R)
    omit = zc.omits(R, "mix")
    omit[64:] = 8
    sup = zc.honest_sup(case, zc.run_ref(case, seeds, None, 0), omit)
    ref = zc.run_ref(case, seeds, omit, 0, 0, 2, sup)
    rc, got = hook(case, seeds, omit, 0, 0, 2, [s[:, :64] for s in sup])
    assert rc == 0
    _compare(got, ref, "sup_r = 64")
    omit[64] = 1  # an opened repetition the supplied rows do not hold
    rc, got = hook(case, seeds, omit, 0, 0, 2, [s[:, :64] for s in sup])
    assert rc == E_ARG and _untouched(got)


# ---------------------------------------------------------------- a chain: a whole program, level by level
def _digests(bufs):
    as_bytes = lambda a: np.ascontiguousarray(a.astype("<u8")).view(np.uint8).reshape(len(a), -1)  # noqa: E731
    return b3_ref.hash_bytes(as_bytes(bufs["pre"])), b3_ref.hash_bytes(as_bytes(bufs["on"]))


def test_chain_vs_oracle_and_proof_commitment(hook, oracle, rule_seeds):
    """every level of a class_mix64 program from production's own records at first_block = 0: the per-repetition streams hash to the
    oracle's commitment and to what Proof.new commits to; the same chain from another first_block and as the verifier follows the
    reference"""
    import reverie_amd as rv
    from reverie_amd import _lib

    prog, wit, wc = cm.class_mix64(cm.MIXED, cm.SEED)
    case = zc.from_program("chain-mixed", prog, wit, wc)
    R = 256
    ref = zc.run_ref(case, rule_seeds, None, 0)
    rc, got = hook(case, rule_seeds, None, 0, 0, 4, key_path=1)
    assert rc == 0
    _compare(got, ref, "chain, first_block 0")
    h, streams, comm = oracle.commit(prog, [], wit, wc, rule_seeds)
    pre, on = _digests(got)
    assert (pre == streams[:, 2]).all() and (on == streams[:, 3]).all()
    c = rv.Circuit(prog, wc)
    L = _lib.lib()
    sh = C.c_void_p()
    w = np.asarray(wit, np.uint64)
    seeds = np.ascontiguousarray(rule_seeds)
    _lib.check(L.rv_shard_commit(c.ctx.handle, c.handle, None, C.c_size_t(0), _p(w), C.c_size_t(len(w)), _p(seeds), C.c_uint32(0), C.c_uint32(R), C.byref(sh)))
    sd = np.zeros((R, 4, 32), np.uint8)
    _lib.check(L.rv_hook_shard_stream_digests(sh, _p(sd)))
    L.rv_shard_destroy(sh)
    c.close()
    assert (sd[:, 2] == pre).all() and (sd[:, 3] == on).all()
    # a window that starts beyond counter byte 14 and crosses a carry into byte 13
    fb = (1 << 17) - 20
    assert fb + case.last_block() > (1 << 17)
    seeds64 = rule_seeds[:64]
    for mode in MODES:
        omit = oracle.challenge(comm)[:64] if mode == "verify" else None
        sup = zc.honest_sup(case, zc.run_ref(case, seeds64, None, fb), omit) if mode == "verify" else None
        ref = zc.run_ref(case, seeds64, omit, fb, sup=sup)
        rc, got = hook(case, seeds64, omit, fb, 0, 1, sup)
        assert rc == 0
        _compare(got, ref, f"chain, first_block {fb}, {mode}")
        assert got["err"][0] == 0


# ---------------------------------------------------------------- refusals
def _patched(case, op, field, value, nth=0):
    g = case.gates.copy()
    at = np.flatnonzero(g["op"] == op)[nth]
    g[field][at] = value
    return g


@pytest.mark.parametrize("mode", MODES)
def test_refusals_leave_every_buffer_untouched(hook, mode):
    R, case = 128, zc.operands(False)
    seeds = _seeds(R)
    V = mode == "verify"
    omit = zc.omits(R, "mix") if V else None
    sup = [np.zeros((max(n, 1), R), np.uint64) for n in (case.n_in, case.n_corr, case.n_rec)] if V else None
    n_ssa, n_rows, row = case.n_ssa, case.n_rows, zr.MASK_ROW
    assert n_rows % 2 == 0
    bad_gates = {
        "Mul with odd m": (zr.MUL, "m", 5), "Random record": (zr.MUL, "op", zr.RANDOM), "B2A record": (zr.ADD, "op", zr.B2A), "unknown op": (zr.CONST, "op", 11),
        "a Mul among the others": (zr.ASSERT, "op", zr.MUL), "a linear gate among the Muls": (zr.MUL, "op", zr.ADD),
        "Mul dst": (zr.MUL, "dst", n_ssa), "Mul a": (zr.MUL, "a", n_ssa), "Mul b": (zr.MUL, "b", n_ssa), "Mul am wire": (zr.MUL, "am", n_ssa),
        "Mul am row": (zr.MUL, "am", row | n_rows), "Mul bm wire": (zr.MUL, "bm", n_ssa), "Mul bm row": (zr.MUL, "bm", row | n_rows),
        "Mul m": (zr.MUL, "m", n_rows - 2 + 2), "Mul eo": (zr.MUL, "eo", case.on_words - 7), "Mul eo wraps": (zr.MUL, "eo", (1 << 64) - 4),
        "Mul ep": (zr.MUL, "ep", case.pre_words),
        "Add dst": (zr.ADD, "dst", n_ssa), "Add a": (zr.ADD, "a", n_ssa), "Add b": (zr.ADD, "b", n_ssa), "Add am": (zr.ADD, "am", row | n_rows),
        "Add bm": (zr.ADD, "bm", n_ssa), "MulConst a": (zr.MULC, "a", n_ssa), "MulConst am": (zr.MULC, "am", n_ssa), "SubConst dst": (zr.SUBC, "dst", n_ssa),
        "Input m": (zr.INPUT, "m", n_rows), "Input dst": (zr.INPUT, "dst", n_ssa), "Input eo": (zr.INPUT, "eo", case.on_words),
        "Input x": (zr.INPUT, "x", case.n_in), "AssertZero a": (zr.ASSERT, "a", n_ssa), "AssertZero am": (zr.ASSERT, "am", row | n_rows),
        "AssertZero eo": (zr.ASSERT, "eo", case.on_words - 7), "Const dst": (zr.CONST, "dst", n_ssa),
    }
    if V:
        bad_gates.update({"Mul x": (zr.MUL, "x", case.n_rec), "Mul xc": (zr.MUL, "xc", case.n_corr), "AssertZero x": (zr.ASSERT, "x", case.n_rec)})
    for name, (op, field, value) in bad_gates.items():
        for nth in (0, -1):
            rc, bufs = hook(case, seeds, omit, 0, 0, 2, sup, gates=_patched(case, op, field, value, nth))
            assert rc == E_ARG and _untouched(bufs), (name, nth, rc)
    lv = case.levels.copy()
    lv[-1, 3] += 1
    lv2 = case.levels.copy()
    lv2[1, 1] = lv2[1, 0] - 1 if lv2[1, 0] else lv2[1, 2] + 1
    for name, kw in {"a level past the records": dict(levels=lv), "a level table out of order": dict(levels=lv2)}.items():
        rc, bufs = hook(case, seeds, omit, 0, 0, 2, sup, **kw)
        assert rc == E_ARG and _untouched(bufs), name
    for qg0, qgn in ((1, 2), (3, 0), (0, 3), (2, 1), (0xFFFFFFFF, 2)):
        rc, bufs = hook(case, seeds, omit, 0, qg0, qgn, sup)
        assert rc == E_ARG and _untouched(bufs), (qg0, qgn)
    for R2 in (16, 48, 8, 260):  # rows of 4, 12 and 2 quad words: no block of 8; more repetitions than a proof has
        o2 = None if omit is None else np.full(R2, 8, np.uint8)
        s2 = [np.zeros((len(s), R2), np.uint64) for s in sup] if V else None
        rc, bufs = hook(case, np.zeros((R2, 16), np.uint8), o2, 0, 0, 1, s2)
        assert rc == E_ARG and _untouched(bufs), R2
    if V:
        o9 = omit.copy()
        o9[R - 1] = 9
        rc, bufs = hook(case, seeds, o9, 0, 0, 2, sup)
        assert rc == E_ARG and _untouched(bufs)
    # counters: the last Mul, or the Input rows' block run, one past the last legal counter
    for fb in (zc.MAX_CTR - case.last_block(), zc.MAX_CTR - 1, zc.MAX_CTR):
        rc, bufs = hook(case, seeds, omit, fb, 0, 2, sup)
        assert rc == E_UNSUPPORTED and _untouched(bufs), fb
    rc, bufs = hook(case, seeds, omit, zc.MAX_CTR + 1, 0, 2, sup)
    assert rc in (E_UNSUPPORTED, E_ARG) and _untouched(bufs)
    rc, bufs = hook(case, seeds, omit, zc.MAX_CTR - 1 - case.last_block(), 0, 2, sup)  # (and the window that just fits is taken)
    assert rc == 0 and not _untouched(bufs)
