"""rv_ops_fold, the host definition of constant folding (no GPU): its records and info against the Python model of tests/fold_ref.py
(which shares no code with it) on the cases of tests/fold_cases.py and 400 generated lists; the forms of the call; the codes;
cleartext evaluation of both lists (every wire's value stays); proofs of folded lists through the CPU oracle; the device's order of
work -- reverie_amd/csrc/fold.h run as plain CPU loops -- in a stand-alone program built with -fsanitize=address,undefined
(tests/fold_model.cpp); the Python face, Block.folded() and the command line's refusals."""
import collections
import ctypes as C
import os
import re
import struct
import subprocess

import numpy as np
import pytest

import eval_ref
import fold_cases as fc
import fold_ref
from conftest import ROOT
from reverie_amd.ops import GF2, OP_DTYPE, Z64, program


@pytest.fixture(scope="module")
def L():
    from reverie_amd import _lib

    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__

        __graft_entry__.build()
    return _lib.lib()


@pytest.fixture(scope="module")
def corpus(L):
    lim = (C.c_uint32 * 5)()
    assert L.rv_hook_fold_limits(lim) == 0
    return fc.corpus(int(lim[1]))


@pytest.fixture(scope="module")
def generated():
    return fc.generated()


_models = {}


def model(case):
    """the Python model's (records, info, kinds) of a case, computed once"""
    if case[0] not in _models:
        _models[case[0]] = fold_ref.fold(case[1])
    return _models[case[0]]


def host_fold(L, ops, wc, out="new", want_info=True):
    """rv_ops_fold through ctypes -> (code, records or None, info dict or None); out: "new", "inplace", None"""
    from reverie_amd import _lib

    ops = np.ascontiguousarray(ops)
    n = len(ops)
    fi = _lib.FoldInfo()
    # (room for one record more: the record behind the list must stay)
    buf = ops.copy() if out == "inplace" else np.full((n + 1) * 24, 0xEE, np.uint8).view(OP_DTYPE) if out == "new" else None
    src = buf if out == "inplace" else ops
    p = lambda a: a.ctypes.data_as(C.c_void_p) if a is not None and a.size else None
    rc = L.rv_ops_fold(p(src), n, int(wc[0]), int(wc[1]), p(buf) if out and n else None, C.byref(fi) if want_info else None)
    if out == "new":
        assert (buf[n:].view(np.uint8) == 0xEE).all()
        buf = buf[:n]
    return rc, buf, {k: int(getattr(fi, k)) for k, _ in fi._fields_} if want_info else None


def test_symbols_exported_and_bound(L):
    import reverie_amd
    from reverie_amd import _lib, fold

    hdr = open(os.path.join(ROOT, "include", "reverie_amd.h")).read()
    for name in ("rv_ops_fold", "rv_ops_fold_device", "rv_hook_fold_limits", "rv_hook_fold_launches"):
        assert name in _lib.SYMBOLS and name in _lib.ARGTYPES
        assert re.search(r"\b" + name + r"\s*\(", hdr), name
    assert C.sizeof(_lib.FoldInfo) == 104
    assert [n for n, _ in _lib.FoldInfo._fields_][3:12] == list(fold_ref.COUNTS)
    assert L.rv_abi_version() == 8  # (calls were added, nothing changed)
    lim = (C.c_uint32 * 5)()
    assert L.rv_hook_fold_limits(lim) == 0 and L.rv_hook_fold_limits(None) == fold_ref.ARG
    assert (lim[0], lim[3]) == (fc.WG, fc.TILE) and lim[1] % lim[0] == 0 and lim[2] >= 1 and lim[4] == 65536
    launches = (C.c_uint64 * 4)()
    assert L.rv_hook_fold_launches(launches) == 0 and L.rv_hook_fold_launches(None) == fold_ref.ARG
    assert reverie_amd.fold_ops is fold.fold_ops


def test_limit_is_read_at_call_time(L, monkeypatch):
    lim = (C.c_uint32 * 5)()
    for value, want in (("3", 3), ("0", 65536), ("x", 65536), ("", 65536), ("4294967296", 65536)):
        monkeypatch.setenv("RV_FOLD_MAX_ROUNDS", value)
        assert L.rv_hook_fold_limits(lim) == 0 and lim[4] == want, value


def test_cases_are_the_issue_s(L, corpus, generated):
    """the case list covers what it says, judged by the Python model alone: every rewrite kind alone in both domains, the chain
    depths, the layer widths around the solo limit, a frontier that crosses the limit both ways, the list lengths around the tile;
    and the generated lists' condition: every rewrite kind and both "left as it is" cases at least 5 times, at least 25 % of the
    lists change and at least 10 % do not"""
    cases = {c[0]: c for c in corpus}
    lim = (C.c_uint32 * 5)()
    assert L.rv_hook_fold_limits(lim) == 0
    solo = int(lim[1])
    for t in "gz":
        for name, kind in (("mul_const", "mul_const"), ("mul_linear_a", "mul_linear"), ("mul_linear_b", "mul_linear"), ("add_addconst_a", "add_addconst"),
                           ("add_addconst_b", "add_addconst"), ("sub_subconst", "sub_subconst"), ("add_const", "linear_const"), ("sub_const", "linear_const"),
                           ("addconst_const", "linear_const"), ("subconst_const", "linear_const"), ("mulconst_const", "linear_const"),
                           ("zero_mulconst", "zero_mulconst"), ("mul_zero_a", "mul_const"), ("mul_zero_b", "mul_const")):
            kinds = model(cases[f"{t}_{name}"])[2]
            assert kinds[3] == f"{t}_{kind}" and [k for k in kinds if k] == [kinds[3]], (t, name, kinds)
        assert model(cases[f"{t}_mul_x_x_known"])[2][3:5] == [f"{t}_mul_const"] * 2 and model(cases[f"{t}_mul_x_x_unknown"])[2][3] is None
        assert model(cases[f"{t}_assert_known_zero"])[1]["asserts_known_zero"] == 2 and model(cases[f"{t}_assert_known_nonzero"])[1]["asserts_known_nonzero"] == 1
    assert model(cases["g_sub_a_known"])[2][3] == "g_sub_addconst" and model(cases["z_sub_a_known"])[2][3] == "left_z_sub_a_known"
    assert model(cases["z_sub_a_known"])[0].tobytes() == cases["z_sub_a_known"][1].tobytes()
    wrap = model(cases["z64_wrap"])[0]
    assert [int(r["imm"]) for r in wrap[4:11]] == [6, (5 - (1 << 63)) & fc.M64, 0, 1, 0, 1, 1 << 63] and int(wrap[13]["imm"]) == fc.M64 - 3
    high = model(cases["gf2_const_high_bits"])
    assert high[0][:3].tobytes() == cases["gf2_const_high_bits"][1][:3].tobytes() and high[2][3:] == ["g_mul_const", "g_mul_linear", "g_add_addconst",
                                                                                                       "g_linear_const", "g_zero_mulconst"]
    assert [int(r["imm"]) for r in high[0][3:]] == [0, 1, 1, 1, 0]
    for name, known, kind in (("b2a_64_known", 1, "b2a_const"), ("b2a_63_known_first_unknown", 0, "left_b2a_unknown_bit"),
                              ("b2a_63_known_last_unknown", 0, "left_b2a_unknown_bit"), ("b2a_0_known", 0, None)):
        out, info, kinds = model(cases[name])
        assert info["b2a_to_const"] == known and kinds[-4] == kind, name
    assert int(model(cases["b2a_64_known"])[0][-4]["imm"]) == 0x8000000000000005 & ~sum(1 << k for k in range(64) if k % 7 == 3)
    assert model(cases["nothing_known"])[0].tobytes() == cases["nothing_known"][1].tobytes() and model(cases["nothing_known"])[1]["n_known"] == 0
    assert model(cases["sizehint_grows"])[1]["n_rewritten"] > 0 and model(cases["unwritten_in_b2a_range"])[1]["b2a_to_const"] == 1
    for name in ("known_then_unknown", "unknown_then_known", "unwritten_reads", "mul_zero_other_input"):
        assert model(cases[name])[1]["n_rewritten"] > 0, name
    assert len(cases["empty"][1]) == 0 and len(cases["one_const"][1]) == 1 and len(cases["one_input"][1]) == 1
    for depth in (1, 2, 63, 64, 65, 3000):
        assert fold_ref.layers(cases[f"known_chain_{depth}"][1])[1] == [1] * depth
    for w in (solo - 1, solo, solo + 1):
        assert fold_ref.layers(cases[f"known_layer_{w}"][1])[1] == [1, w]
    wn = fold_ref.layers(cases["widen_past_solo_and_narrow"][1])[1]
    assert wn == [1 << k for k in range(12)] + [1 << k for k in range(10, -1, -1)] and max(wn) > solo > min(wn)
    assert [len(cases[f"length_{n}"][1]) for n in (255, 256, 257, 513)] == [255, 256, 257, 513]
    # the generated lists
    assert len(generated) == 400 and all(1 <= len(c[1]) <= 300 + 110 for c in generated)
    kinds, changed = collections.Counter(), 0
    for case in generated:
        out, _, k = model(case)
        kinds.update(x for x in k if x)
        changed += out.tobytes() != case[1].tobytes()
    assert all(kinds[k] >= 5 for k in fold_ref.KINDS), kinds
    assert changed >= 100 and len(generated) - changed >= 40, changed


def check_against_model(L, case):
    name, ops, wc = case
    want_ops, want_info, _ = model(case)
    rc, out, info = host_fold(L, ops, wc)
    assert rc == 0, (name, rc)
    assert out.tobytes() == want_ops.tobytes(), name
    assert info == want_info, (name, info, want_info)
    return out, info


def test_corpus_equals_model(L, corpus):
    for case in corpus:
        check_against_model(L, case)


def test_generated_lists(L, generated):
    """rv_ops_fold is the model's output; every folded list is its own fixed point; a rewritten record is clean"""
    for case in generated:
        name, ops, wc = case
        out, info = check_against_model(L, case)
        rc, again, info2 = host_fold(L, out, wc)
        assert rc == 0 and again.tobytes() == out.tobytes() and info2["n_rewritten"] == 0 and info2["n_known"] == info["n_known"], name
        new = out[np.flatnonzero([a.tobytes() != b.tobytes() for a, b in zip(out, ops)])]
        assert (new["reserved"] == 0).all() and (new["b"] == 0).all() and (new["a"][new["opcode"] == 9] == 0).all(), name
        assert (new["imm"][new["domain"] == 0] <= 1).all() and (new["domain"] <= 1).all() and np.isin(new["opcode"], (3, 5, 7, 9)).all(), name


def test_forms_of_the_call(L, corpus):
    """in place equals out of place; the counting call gives the full call's numbers and writes nothing; info may be NULL; folding
    the result changes nothing"""
    for case in corpus:
        name, ops, wc = case
        want_ops, want_info, _ = model(case)
        rc, out, info = host_fold(L, ops, wc, out="inplace")
        assert rc == 0 and out.tobytes() == want_ops.tobytes() and info == want_info, name
        rc, _, info = host_fold(L, ops, wc, out=None)
        assert rc == 0 and info == want_info, name
        rc, out, _ = host_fold(L, ops, wc, want_info=False)
        assert rc == 0 and out.tobytes() == want_ops.tobytes(), name
        rc, again, info2 = host_fold(L, want_ops, wc)
        assert rc == 0 and again.tobytes() == want_ops.tobytes() and info2["n_rewritten"] == 0, name


def test_argument_errors(L):
    ops = program([GF2.Const(0, 1), GF2.Mul(1, 0, 0)])
    p = ops.ctypes.data_as(C.c_void_p)
    assert L.rv_ops_fold(None, 2, 0, 2, None, None) == fold_ref.ARG
    assert L.rv_ops_fold(None, 0, 0, 0, None, None) == 0
    assert L.rv_ops_fold(p, 2, 0, 2, None, None) == 0  # (out and info are optional)
    # an overlap that is not the in-place form
    both = np.concatenate([ops, ops])
    q = C.c_void_p(both.ctypes.data + 24)
    assert L.rv_ops_fold(both.ctypes.data_as(C.c_void_p), 2, 0, 2, q, None) == fold_ref.ARG
    assert both.tobytes() == np.concatenate([ops, ops]).tobytes()


@pytest.mark.parametrize("case", fc.error_cases(), ids=[c[0] for c in fc.error_cases()])
def test_codes(L, case):
    """the codes are rv_ops_prune's on the same lists (the first bad op in op order); nothing is written"""
    from reverie_amd import _lib

    name, ops, wc = case
    n_out, pi = C.c_size_t(), _lib.PruneInfo()
    want = L.rv_ops_prune(ops.ctypes.data_as(C.c_void_p), len(ops), wc[0], wc[1], None, 0, None, 0, None, 0, C.byref(n_out), None, C.byref(pi))
    assert want != 0 and want == fold_ref.check(ops, wc), name
    rc, out, _ = host_fold(L, ops, wc)
    assert rc == want and (out.view(np.uint8) == 0xEE).all(), (name, rc, want)
    assert host_fold(L, ops, wc, out=None)[0] == want and host_fold(L, ops, wc, out="inplace")[1].tobytes() == ops.tobytes()


# ---- values are kept ----
def witnesses(ops, rng, count=4):
    n_g = int(np.count_nonzero((ops["domain"] == 0) & (ops["opcode"] == 0)))
    n_z = int(np.count_nonzero((ops["domain"] == 1) & (ops["opcode"] == 0)))
    z = rng.integers(0, 1 << 63, (count, n_z), dtype=np.uint64) * np.uint64(2) + rng.integers(0, 2, (count, n_z), dtype=np.uint64)
    z[0] = 0  # (zeros and small values make products and sums vanish)
    z[1] = rng.integers(0, 3, n_z)
    return rng.integers(0, 2, (count, n_g), dtype=np.uint8), z


def test_values_are_kept(L, corpus, generated):
    """cleartext evaluation of the original and of the folded list: identical GF(2) and Z64 wire vectors, failing-assertion counts
    and first failing op, for 4 random witnesses per list (a Random is evaluated as Const 0)"""
    rng = np.random.default_rng(24)
    for case in corpus + generated:
        name, ops, wc = case
        if len(ops) == 0 or name == "compact_sparse":  # (the model evaluator holds every wire index: 2^24 of them there)
            continue
        folded = model(case)[0].copy()
        ops = ops.copy()
        for lst in (ops, folded):
            randoms = (lst["domain"] <= 1) & (lst["opcode"] == 1)
            lst["opcode"][randoms], lst["imm"][randoms] = 9, 0
        g, z = witnesses(ops, rng)
        a = eval_ref.evaluate(ops, wc, g, z)
        b = eval_ref.evaluate(folded, wc, g, z)
        assert (a[0] == b[0]).all() and (a[1] == b[1]).all(), name
        assert (a[2] == b[2]).all() and (a[3] == b[3]).all(), name


# ---- proofs: the layout of a proof's bytes is test_prune_host.py's; a folded Mul or B2A stops contributing as a dropped one does ----
ONLINE_REPS = 40


def dropped_bytes(gf2_mul, z64_mul, b2a):
    gf2_recon, gf2_corr = gf2_mul + 127 * b2a, gf2_mul + 63 * b2a
    assert gf2_recon % 8 == 0 and gf2_corr % 8 == 0  # (fold_cases.proof_programs keeps the bit vectors whole bytes)
    return ONLINE_REPS * (gf2_recon // 8 + gf2_corr // 8 + 16 * z64_mul + 8 * b2a)


@pytest.mark.parametrize("case", fc.proof_programs(), ids=[c[0] for c in fc.proof_programs()])
def test_proof_of_folded_list(L, oracle, rule_seeds, case):
    """the oracle's proof of the folded list verifies against the folded list, is shorter than the proof of the original by exactly
    what the folded Muls and B2As account for, and is not accepted for the original; the proof of fold-then-prune is shorter again"""
    from reverie_amd import _lib

    name, ops, wc, wit_g, wit_z, counts = case
    rc, folded, info = host_fold(L, ops, wc)
    assert rc == 0 and folded.tobytes() == fold_ref.fold(ops)[0].tobytes()
    assert (info["gf2_mul_to_const"] + info["gf2_mul_to_linear"], info["z64_mul_to_const"] + info["z64_mul_to_linear"], info["b2a_to_const"]) == counts
    g, z = np.asarray([wit_g], np.uint8), np.asarray([wit_z], np.uint64)
    assert int(eval_ref.evaluate(ops, wc, g, z)[2][0]) == 0 and int(eval_ref.evaluate(folded, wc, g, z)[2][0]) == 0
    full = oracle.prove(ops, wit_g, wit_z, wc, rule_seeds, threads=2)
    short = oracle.prove(folded, wit_g, wit_z, wc, rule_seeds, threads=2)
    assert oracle.verify(folded, wc, short, threads=2, strict=True)
    assert oracle.verify(ops, wc, full, threads=2, strict=True)
    assert len(full) - len(short) == dropped_bytes(*counts) > 0, (name, len(full), len(short))
    try:
        crossed = oracle.verify(ops, wc, short, threads=2, strict=True)
    except oracle.OracleError:
        crossed = False
    assert not crossed  # the proof of the folded list is not a proof of the original
    pruned, n_out, pi = np.empty_like(folded), C.c_size_t(), _lib.PruneInfo()
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    assert L.rv_ops_prune(p(folded), len(folded), wc[0], wc[1], None, 0, None, 0, p(pruned), len(pruned), C.byref(n_out), None, C.byref(pi)) == 0
    pruned = pruned[:n_out.value].copy()
    assert pi.dropped_gf2_mul + pi.dropped_z64_mul > 0
    shorter = oracle.prove(pruned, wit_g, wit_z, wc, rule_seeds, threads=2)
    assert oracle.verify(pruned, wc, shorter, threads=2, strict=True) and len(shorter) < len(short)
    assert len(short) - len(shorter) == dropped_bytes(pi.dropped_gf2_mul, pi.dropped_z64_mul, pi.dropped_b2a)


# ---- the device's order of work, under the sanitizers ----
def to_file(case):
    name, ops, wc = case[:3]
    return struct.pack("<3Q", len(ops), wc[0], wc[1]) + np.ascontiguousarray(ops).tobytes()


def fnv(data: bytes) -> int:
    h = 1469598103934665603
    for b in data:
        h = ((h ^ b) * 1099511628211) & 0xFFFFFFFFFFFFFFFF
    return h


def test_model_under_sanitizers(L, corpus, generated, tmp_path):
    """the stand-alone program: clean under AddressSanitizer and UBSan; for every case the device's order of work gives rv_ops_fold's
    code, records and info (the program compares), the layer count is the longest known chain of the Python model, the solo loop and
    the wide rounds are taken where the widths say, and the bytes are the Python model's (compared here, by digest)"""
    exe = str(tmp_path / "fold_model")
    csrc = os.path.join(ROOT, "reverie_amd", "csrc")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", csrc,
                           os.path.join(ROOT, "tests", "fold_model.cpp"), os.path.join(csrc, "fold.cpp"), "-o", exe])
    lim = (C.c_uint32 * 5)()
    assert L.rv_hook_fold_limits(lim) == 0
    solo_limit = int(lim[1])
    whole = [c + (0,) for c in corpus] + [c + (0,) for c in generated[:80]] + [c + (fold_ref.check(c[1], c[2]),) for c in fc.error_cases()]
    paths = []
    for k, case in enumerate(whole):
        path = str(tmp_path / f"{k:03d}-{case[0]}.ops")
        with open(path, "wb") as f:
            f.write(to_file(case))
        paths.append(path)
    run = subprocess.run([exe] + paths, capture_output=True, text=True)
    assert run.returncode == 0 and "Sanitizer" not in run.stderr and "runtime error" not in run.stderr, (run.stdout[-2000:], run.stderr[-2000:])
    lines = run.stdout.split("\n")
    assert lines[-2] == "bad 0"
    answers = {ln.split()[0]: ln.split()[1:] for ln in lines if re.match(r"\d\d\d-", ln)}
    assert len(answers) == len(whole)
    seen_solo = seen_wide = 0
    for k, case in enumerate(whole):
        rc, n_known, layers, solo, wide, digest = answers[f"{k:03d}-{case[0]}.ops"]
        assert int(rc) == case[3], case[0]
        if case[3]:
            continue
        want_ops, want_info, _ = model(case)
        layer, widths = fold_ref.layers(case[1])
        assert int(n_known) == want_info["n_known"] == len(layer) and int(layers) == len(widths), case[0]
        assert int(solo) == sum(w <= solo_limit for w in widths) and int(wide) == sum(w > solo_limit for w in widths), case[0]
        assert int(digest, 16) == fnv(want_ops.tobytes()), case[0]
        seen_solo, seen_wide = seen_solo + int(solo), seen_wide + int(wide)
    assert seen_solo and seen_wide
    # the bound: the depth-65 chain stops after 3 layers, as the device call does before it falls back
    chain = [p for p in paths if p.endswith("known_chain_65.ops")]
    run = subprocess.run([exe, "--max-rounds", "3"] + chain, capture_output=True, text=True)
    assert run.returncode == 0 and "Sanitizer" not in run.stderr, run.stderr[-2000:]
    assert run.stdout.split("\n")[0].split()[3:] == ["3", "3", "0", "fallback"]


# ---- the Python face ----
def test_python_face_on_host_arrays(L, corpus):
    import reverie_amd as rv

    case = {c[0]: c for c in corpus}["z64_wrap"]
    name, ops, wc = case
    want_ops, want_info, _ = model(case)
    out, info = rv.fold_ops(ops, wc)
    assert out.dtype == OP_DTYPE and out.tobytes() == want_ops.tobytes() and info == want_info and out is not ops
    none, info2 = rv.fold_ops(ops, wc, count_only=True)
    assert none is None and info2 == want_info
    tuples = [tuple(r) for r in ops.tolist()]
    assert rv.fold_ops(tuples)[0].tobytes() == want_ops.tobytes()  # (wire counts from largest_wires)
    mine = ops.copy()
    same, info3 = rv.fold_ops(mine, wc, inplace=True)
    assert same is mine and mine.tobytes() == want_ops.tobytes() and info3 == want_info
    with pytest.raises(ValueError):
        rv.fold_ops(tuples, inplace=True)
    out, info = rv.fold_ops([])
    assert len(out) == 0 and info["n_ops"] == 0
    with pytest.raises(rv.ReverieError) as e:
        rv.fold_ops(ops, (1, 0))
    assert e.value.code == fold_ref.WIRE_OOB


def test_block_folded(L):
    """a block whose constants are its own (no head): the ports, counts and outputs stay, the records are the model's, and the
    netlist linked from it evaluates to the same outputs"""
    import reverie_amd as rv

    ops = program([GF2.Input(0), GF2.Input(1), GF2.Const(2, 1), GF2.Const(3, 0), GF2.Mul(4, 0, 2), GF2.Mul(5, 1, 3), GF2.Mul(6, 0, 1), GF2.Add(7, 4, 5),
                   GF2.Add(8, 7, 6), GF2.Sub(9, 2, 8)])
    block = rv.Block(ops, (0, 10), outputs=[8, 9])
    folded = block.folded()
    want, want_info, _ = fold_ref.fold(ops)
    assert folded.ops.tobytes() == want.tobytes() and folded.fold_info == want_info and want_info["gf2_mul_to_linear"] == 1
    assert (folded.n_ports, folded.wire_counts, folded.outputs, folded.on_device) == (block.n_ports, block.wire_counts, block.outputs, False)
    pruned = folded.pruned()
    assert len(pruned.ops) < len(folded.ops) and pruned.outputs == block.outputs


def test_command_line_refusals(L, tmp_path, capsys):
    from reverie_amd.__main__ import main

    prog = str(tmp_path / "p.rvops")
    program([GF2.Input(0), GF2.Const(1, 1), GF2.Mul(2, 0, 1), GF2.AssertZero(2)]).tofile(prog)
    base = ["--operation", "convert", "--program-path", prog, "--program-format", "rvops", "--output-path", str(tmp_path / "o.rvops"), "--output-format",
            "rvops", "--fold"]
    for extra in (["--window-mb", "1"], ["--compact-windows"], ["--prune-windows"]):
        with pytest.raises(SystemExit) as e:
            main(base + extra)
        assert e.value.code == 2
        assert "--fold needs a source that is read whole" in capsys.readouterr().err
    # and without them it folds on the host, before anything else: the counts on stderr
    assert main(base) == 0
    err = capsys.readouterr().err
    assert "fold: 4 ops, 1 rewritten" in err
    want = program([GF2.Input(0), GF2.Const(1, 1), GF2.MulConst(2, 0, 1), GF2.AssertZero(2)])
    assert np.fromfile(str(tmp_path / "o.rvops"), OP_DTYPE).tobytes() == want.tobytes()
    # fold, then prune: the Const nothing reads any more goes
    assert main(base + ["--prune"]) == 0
    err = capsys.readouterr().err
    assert err.index("fold:") < err.index("prune: 4 ops -> 3")
    assert np.fromfile(str(tmp_path / "o.rvops"), OP_DTYPE).tobytes() == want[[0, 2, 3]].tobytes()


def test_fold_is_refused_on_pieces(L):
    from reverie_amd import stream

    pieces = lambda: iter([(program([Z64.Input(0)]), None)])
    for fn, args in ((stream.prove_streaming_pieces, (pieces, [], [5], (1, 0))), (stream.verify_streaming_pieces, (pieces, (1, 0), b"")),
                     (stream.evaluate_streaming_pieces, (pieces, [], [5], (1, 0)))):
        with pytest.raises(ValueError) as e:
            fn(*args, fold=True)
        assert "a window's unwritten index is not the list's" in str(e.value)
