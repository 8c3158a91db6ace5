"""rv_ops_prune, the host definition of pruning (no GPU): its records, old_index and info against the two Python models of
tests/prune_ref.py (which share no code with it) on the cases of tests/prune_cases.py and 400 generated lists; the forms of the call;
the codes; proofs of pruned lists through the CPU oracle; cleartext evaluation of both lists; the device's order of work --
reverie_amd/csrc/prune.h run as plain CPU loops -- in a stand-alone program built with -fsanitize=address,undefined
(tests/prune_model.cpp); the Python face, Block.pruned() and the command line's refusals."""
import ctypes as C
import os
import re
import struct
import subprocess

import numpy as np
import pytest

import compact_cases
import eval_ref
import prune_cases as pc
import prune_ref
from conftest import ROOT
from reverie_amd.ops import GF2, OP_DTYPE, program


@pytest.fixture(scope="module")
def L():
    from reverie_amd import _lib

    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__

        __graft_entry__.build()
    return _lib.lib()


_models = {}


def model(case):
    """the sweep model's (kept records, old_index, info) of a case, computed once"""
    name, ops, wc, og, oz = case[:5]
    if name not in _models:
        keep, info = prune_ref.sweep(ops, og, oz)
        _models[name] = (ops[keep], np.flatnonzero(keep).astype(np.uint32), info)
    return _models[name]


@pytest.fixture(scope="module")
def corpus():
    return pc.corpus()


@pytest.fixture(scope="module")
def generated():
    return pc.generated()


def host_prune(L, ops, wc, og=(), oz=(), out="new", cap=None, want_old=True):
    """rv_ops_prune through ctypes -> (code, kept records or None, old_index or None, info dict, n_out); out: "new", "inplace", None"""
    from reverie_amd import _lib

    ops = np.ascontiguousarray(ops)
    g, z = np.asarray(og, np.uint32), np.asarray(oz, np.uint32)
    pi, n_out = _lib.PruneInfo(), C.c_size_t(12345)
    cap = len(ops) if cap is None else cap
    # (room for one record more than the capacity: a capacity of 0 still is a call that writes, and the record behind must stay)
    buf = ops.copy() if out == "inplace" else np.full((cap + 1) * 24, 0xEE, np.uint8).view(OP_DTYPE) if out == "new" else None
    src = buf if out == "inplace" else ops
    old = np.full(cap + 1, 0xEEEEEEEE, np.uint32) if want_old and out else None
    p = lambda a: a.ctypes.data_as(C.c_void_p) if a is not None and a.size else None
    rc = L.rv_ops_prune(p(src), len(ops), int(wc[0]), int(wc[1]), p(g), g.size, p(z), z.size, p(buf) if out else None, cap, C.byref(n_out), p(old),
                        C.byref(pi))
    info = {n: int(getattr(pi, n)) for n, _ in pi._fields_}
    if out == "new":
        assert (buf[cap:].view(np.uint8) == 0xEE).all() and (old is None or old[cap] == 0xEEEEEEEE)
        buf, old = buf[:cap], old[:cap] if old is not None else None
    return rc, buf, old, info, int(n_out.value)


def test_symbols_exported_and_bound(L):
    import reverie_amd
    from reverie_amd import _lib, prune

    hdr = open(os.path.join(ROOT, "include", "reverie_amd.h")).read()
    for name in ("rv_ops_prune", "rv_ops_prune_device", "rv_hook_prune_limits", "rv_hook_prune_launches"):
        assert name in _lib.SYMBOLS and name in _lib.ARGTYPES
        assert re.search(r"\b" + name + r"\s*\(", hdr), name
    assert C.sizeof(_lib.PruneInfo) == 96
    assert L.rv_abi_version() == 8  # (calls were added, nothing changed)
    lim = (C.c_uint32 * 5)()
    assert L.rv_hook_prune_limits(lim) == 0 and L.rv_hook_prune_limits(None) == prune_ref.ARG
    assert (lim[0], lim[1], lim[3]) == (pc.WG, pc.SOLO_LIMIT, pc.TILE) and lim[2] >= 1 and lim[4] == 65536
    assert reverie_amd.prune_ops is prune.prune_ops


def test_limit_is_read_at_call_time(L, monkeypatch):
    lim = (C.c_uint32 * 5)()
    for value, want in (("3", 3), ("0", 65536), ("x", 65536), ("", 65536), ("4294967296", 65536)):
        monkeypatch.setenv("RV_PRUNE_MAX_ROUNDS", value)
        assert L.rv_hook_prune_limits(lim) == 0 and lim[4] == want, value


def test_cases_are_the_issue_s(corpus):
    """the case list covers what it says: the chain depths, the layer widths around the wavefront, the workgroup and the solo limit, a
    frontier that widens past the limit and narrows again, the list lengths around the tiles, both image alignments"""
    cases = {c[0]: c for c in corpus}
    widths = {}
    for name, c in cases.items():
        if name.startswith(("dead_", "widen", "alignments")):
            widths[name] = prune_ref.peel(c[1], c[3], c[4])[1]["widths"]
    for depth in (1, 2, 5000):
        assert widths[f"dead_chain_{depth}"] == [1] * depth
    for w in (1, 64, 65, 256, 257, 1024, 1025, 70000):
        assert widths[f"dead_layer_{w}"] == [w]
    wn = widths["widen_past_solo_and_narrow"]
    assert wn[:12] == [1 << k for k in range(12)] and wn[12:] == [1, 1, 1, 1] and max(wn) > pc.SOLO_LIMIT
    assert {len(cases[f"length_{n}"][1]) for n in (1, 255, 256, 257, 2047, 2048, 2049, 70000)} == {1, 255, 256, 257, 2047, 2048, 2049, 70000}
    assert len(cases["empty"][1]) == 0
    # kept records before each tile of 256: an odd count puts the tile's image 8 bytes off
    keep = prune_ref.sweep(cases["alignments"][1])[0]
    firsts = [int(np.count_nonzero(keep[:t])) & 1 for t in range(0, len(keep), pc.TILE)]
    assert set(firsts) == {0, 1}
    b2a = prune_ref.sweep(cases["b2a_ranges"][1])[1]
    assert b2a["dropped_b2a"] == 3 and b2a["n_kept"] < len(cases["b2a_ranges"][1])


def check_against_model(L, case):
    name, ops, wc, og, oz = case
    want_ops, want_old, want_info = model(case)
    rc, out, old, info, n_out = host_prune(L, ops, wc, og, oz)
    assert rc == 0, (name, rc)
    assert n_out == len(want_ops) == info["n_kept"], name
    assert out[:n_out].tobytes() == want_ops.tobytes(), name
    assert (old[:n_out] == want_old).all(), name
    assert info == want_info, (name, info, want_info)
    assert (out[n_out:].view(np.uint8) == 0xEE).all() and (old[n_out:] == 0xEEEEEEEE).all(), name  # nothing behind the kept records
    return out[:n_out], old[:n_out], info


def test_corpus_equals_sweep_model(L, corpus):
    for case in corpus:
        check_against_model(L, case)


def test_generated_lists(L, generated):
    """the issue's generator: rv_ops_prune is the sweep model's output, the peeling model keeps the same set, every pruned list is its
    own fixed point"""
    deepest = 0
    for case in generated:
        name, ops, wc, og, oz = case
        out, _, info = check_against_model(L, case)
        keep2, info2 = prune_ref.peel(ops, og, oz)
        assert ops[keep2].tobytes() == out.tobytes(), name
        assert {k: info2[k] for k in info if k not in ("device_rounds", "on_device")} == {k: v for k, v in info.items() if k not in ("device_rounds", "on_device")}
        deepest = max(deepest, info2["device_rounds"])
        rc, again, _, info3, n3 = host_prune(L, out, wc, og, oz)
        assert rc == 0 and n3 == len(out) and info3["n_dropped"] == 0 and again[:n3].tobytes() == out.tobytes(), name
    assert 5 <= deepest <= 200  # (dead cones of some depth do open; the issue's run saw 27)


def test_forms_of_the_call(L, corpus):
    """in place equals out of place; the counting call gives the full call's numbers and writes nothing; a short capacity is refused
    and leaves `out` untouched; pruning the result drops nothing"""
    for case in corpus:
        name, ops, wc, og, oz = case
        if len(ops) > 5000:
            continue
        want_ops, want_old, want_info = model(case)
        rc, out, old, info, n_out = host_prune(L, ops, wc, og, oz, out="inplace")
        assert rc == 0 and n_out == len(want_ops) and out[:n_out].tobytes() == want_ops.tobytes() and (old[:n_out] == want_old).all(), name
        assert out[n_out:].tobytes() == ops[n_out:].tobytes(), name  # (the tail of an in-place list is left as it was)
        rc, _, _, info, n_out = host_prune(L, ops, wc, og, oz, out=None)
        assert rc == 0 and n_out == len(want_ops) and info == want_info, name
        if len(want_ops):
            rc, out, old, _, _ = host_prune(L, ops, wc, og, oz, cap=len(want_ops) - 1)
            assert rc == prune_ref.ARG and (out.view(np.uint8) == 0xEE).all() and (old == 0xEEEEEEEE).all(), name
        rc, out, _, _, n_out = host_prune(L, ops, wc, og, oz, cap=len(want_ops), want_old=False)  # exactly enough; no old_index
        assert rc == 0 and out.tobytes() == want_ops.tobytes(), name
        rc, again, _, info2, n2 = host_prune(L, want_ops, wc, og, oz)
        assert rc == 0 and n2 == len(want_ops) and info2["n_dropped"] == 0 and again[:n2].tobytes() == want_ops.tobytes(), name


def test_argument_errors(L):
    ops = program([GF2.Input(0), GF2.Mul(1, 0, 0)])
    n = C.c_size_t()
    p = ops.ctypes.data_as(C.c_void_p)
    assert L.rv_ops_prune(None, 2, 0, 2, None, 0, None, 0, None, 0, C.byref(n), None, None) == prune_ref.ARG
    assert L.rv_ops_prune(p, 2, 0, 2, None, 1, None, 0, None, 0, C.byref(n), None, None) == prune_ref.ARG
    assert L.rv_ops_prune(p, 2, 0, 2, None, 0, None, 1, None, 0, C.byref(n), None, None) == prune_ref.ARG
    assert L.rv_ops_prune(None, 0, 0, 0, None, 0, None, 0, None, 0, C.byref(n), None, None) == 0 and n.value == 0
    assert L.rv_ops_prune(p, 2, 0, 2, None, 0, None, 0, None, 0, None, None, None) == 0  # (n_out and info are optional)
    # an overlap that is not the in-place form
    both = np.concatenate([ops, ops])
    q = C.c_void_p(both.ctypes.data + 24)
    assert L.rv_ops_prune(both.ctypes.data_as(C.c_void_p), 2, 0, 2, None, 0, None, 0, q, 2, C.byref(n), None, None) == prune_ref.ARG
    assert both.tobytes() == np.concatenate([ops, ops]).tobytes()


@pytest.mark.parametrize("case", pc.error_cases(), ids=[c[0] for c in pc.error_cases()])
def test_codes(L, case):
    """the codes are rv_ops_compact_wires' on the same lists (the first bad op in op order), then RV_E_ARG for an output out of range;
    nothing is written"""
    from reverie_amd import _lib

    name, ops, wc, og, oz, code = case
    ci = _lib.CompactInfo()
    scratch = np.empty_like(ops)
    compact_rc = L.rv_ops_compact_wires(ops.ctypes.data_as(C.c_void_p), len(ops), wc[0], wc[1], scratch.ctypes.data_as(C.c_void_p), C.byref(ci))
    want = code if code is not None and compact_rc == 0 else compact_rc
    assert want != 0 and want == prune_ref.check(ops, wc, og, oz), name
    rc, out, old, _, n_out = host_prune(L, ops, wc, og, oz)
    assert rc == want, (name, rc, want)
    assert (out.view(np.uint8) == 0xEE).all() and (old == 0xEEEEEEEE).all() and n_out == 12345, name
    assert host_prune(L, ops, wc, og, oz, out=None)[0] == want and host_prune(L, ops, wc, og, oz, out="inplace")[1].tobytes() == ops.tobytes()


# ---- proofs: the layout of a proof's bytes, per online repetition (40 of them; SURVEY §8: R reconstructions, C corrections) ----
#   GF(2): one reconstruction bit per Mul and AssertZero and one correction bit per Mul, each vector packed 8 bits to the byte;
#          a B2A adds 127 reconstruction bits and 63 correction bits (its 63-Mul adder and 64 recorded reconstructions)
#   Z64:   8 bytes of reconstruction per Mul and AssertZero and 8 bytes of correction per Mul; a B2A adds 8 bytes of correction
# A Random, an Input nobody reads and the linear ops cost masks and time, not proof bytes.
ONLINE_REPS = 40


def dropped_bytes(info):
    gf2_recon = info["dropped_gf2_mul"] + 127 * info["dropped_b2a"]
    gf2_corr = info["dropped_gf2_mul"] + 63 * info["dropped_b2a"]
    assert gf2_recon % 8 == 0 and gf2_corr % 8 == 0  # (prune_cases.proof_programs keeps the bit vectors whole bytes)
    return ONLINE_REPS * (gf2_recon // 8 + gf2_corr // 8 + 16 * info["dropped_z64_mul"] + 8 * info["dropped_b2a"])


@pytest.mark.parametrize("case", pc.proof_programs(), ids=[c[0] for c in pc.proof_programs()])
def test_proof_of_pruned_list(L, oracle, rule_seeds, case):
    """the oracle's proof of the pruned list verifies against the pruned list, is strictly shorter than the proof of the original, by
    exactly what the dropped ops account for, and is not accepted for the original"""
    name, ops, wc, wit_g, wit_z = case
    rc, out, _, info, n_out = host_prune(L, ops, wc)
    assert rc == 0 and info["n_dropped"] > 0 and info["dropped_gf2_random"] + info["dropped_z64_random"] > 0
    assert {"gf2": info["dropped_gf2_mul"] == 16, "z64": info["dropped_z64_mul"] == 2,
            "mixed": (info["dropped_gf2_mul"], info["dropped_z64_mul"], info["dropped_b2a"]) == (65, 1, 1)}[name]
    pruned = out[:n_out].copy()
    full = oracle.prove(ops, wit_g, wit_z, wc, rule_seeds, threads=2)
    short = oracle.prove(pruned, wit_g, wit_z, wc, rule_seeds, threads=2)
    assert oracle.verify(pruned, wc, short, threads=2, strict=True)
    assert oracle.verify(ops, wc, full, threads=2, strict=True)
    assert len(short) < len(full)
    assert len(full) - len(short) == dropped_bytes(info), (name, len(full), len(short))
    try:
        crossed = oracle.verify(ops, wc, short, threads=2, strict=True)
    except oracle.OracleError:
        crossed = False
    assert not crossed  # the proof of the pruned list is not a proof of the original


@pytest.mark.parametrize("case", pc.proof_programs(), ids=[c[0] for c in pc.proof_programs()])
def test_evaluation_agrees(L, case):
    """cleartext evaluation gives the same number of failing assertions on both lists, for a witness that passes and one that fails;
    the first failing op of the pruned list maps to the original's through old_index"""
    name, ops, wc, wit_g, wit_z = case
    rc, out, old, _, n_out = host_prune(L, ops, wc)
    pruned, old = out[:n_out].copy(), old[:n_out]
    # (a Random has no cleartext value: the model evaluates it as Const 0 -- in these programs every Random is dead)
    ops = ops.copy()
    for lst in (ops, pruned):
        lst["opcode"][(lst["domain"] <= 1) & (lst["opcode"] == 1)] = 9
    for fail in (False, True):
        g, z = list(wit_g), list(wit_z)
        if fail:
            if g:
                g[0] ^= 1
            else:
                z[0] += 1
        a = eval_ref.evaluate(ops, wc, np.asarray(g, np.uint8) if g else None, np.asarray(z, np.uint64) if z else None)
        b = eval_ref.evaluate(pruned, wc, np.asarray(g, np.uint8) if g else None, np.asarray(z, np.uint64) if z else None)
        assert int(a[2][0]) == int(b[2][0]) and (int(a[2][0]) > 0) == fail, (name, fail)
        if fail:
            assert int(old[int(b[3][0])]) == int(a[3][0]), name
        else:
            assert int(a[3][0]) == int(b[3][0]) == -1, name


def to_file(case):
    name, ops, wc, og, oz = case[:5]
    g, z = np.asarray(og, np.uint32), np.asarray(oz, np.uint32)
    return struct.pack("<5Q", len(ops), wc[0], wc[1], g.size, z.size) + np.ascontiguousarray(ops).tobytes() + g.tobytes() + z.tobytes()


def fnv(data: bytes) -> int:
    a = np.frombuffer(data, np.uint8)
    h = 1469598103934665603
    for b in a.tolist():
        h = ((h ^ b) * 1099511628211) & 0xFFFFFFFFFFFFFFFF
    return h


def test_model_under_sanitizers(L, corpus, generated, tmp_path):
    """the stand-alone program: clean under AddressSanitizer and UBSan; for every case the device's order of work gives rv_ops_prune's
    code, records, old_index and info (the program compares), the layer counts are the peeling model's, the solo loop and the wide
    rounds are taken where the widths say, and the bytes are the sweep model's (compared here, by digest)"""
    exe = str(tmp_path / "prune_model")
    csrc = os.path.join(ROOT, "reverie_amd", "csrc")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", csrc,
                           os.path.join(ROOT, "tests", "prune_model.cpp"), os.path.join(csrc, "prune.cpp"), "-o", exe])
    whole = [c + (0,) for c in corpus] + [c + (0,) for c in generated[:60]] + [c[:5] + (prune_ref.check(c[1], c[2], c[3], c[4]),) for c in pc.error_cases()]
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
        rc, n_kept, layers, solo, wide, digest = answers[f"{k:03d}-{case[0]}.ops"]
        assert int(rc) == case[5], case[0]
        if case[5]:
            continue
        want_ops = model(case)[0]
        widths = prune_ref.peel(case[1], case[3], case[4])[1]["widths"]
        assert int(n_kept) == len(want_ops) and int(layers) == len(widths), case[0]
        assert int(solo) == sum(w <= pc.SOLO_LIMIT for w in widths) and int(wide) == sum(w > pc.SOLO_LIMIT for w in widths), case[0]
        assert len(want_ops) > 3000 or int(digest, 16) == fnv(want_ops.tobytes()), case[0]
        seen_solo, seen_wide = seen_solo + int(solo), seen_wide + int(wide)
    assert seen_solo and seen_wide
    # the bound: the depth-5 000 chain stops after 3 layers, as the device call does before it falls back
    chain = [p for p in paths if p.endswith("dead_chain_5000.ops")]
    run = subprocess.run([exe, "--max-rounds", "3"] + chain, capture_output=True, text=True)
    assert run.returncode == 0 and "Sanitizer" not in run.stderr, run.stderr[-2000:]
    assert run.stdout.split("\n")[0].split()[3:] == ["3", "3", "0", "fallback"]


def test_python_face_on_host_arrays(L, corpus):
    import reverie_amd as rv

    case = {c[0]: c for c in corpus}["b2a_output"]
    name, ops, wc, og, oz = case
    want_ops, want_old, want_info = model(case)
    out, info, old = rv.prune_ops(ops, wc, og, oz)
    assert out.dtype == OP_DTYPE and out.tobytes() == want_ops.tobytes() and (old == want_old).all() and info == want_info
    none, info2, none2 = rv.prune_ops(ops, wc, og, oz, count_only=True)
    assert none is None and none2 is None and info2 == want_info
    tuples = [tuple(r) for r in ops.tolist()]
    assert rv.prune_ops(tuples, outputs_gf2=og, outputs_z64=oz)[0].tobytes() == want_ops.tobytes()  # (wire counts from largest_wires)
    out, info, old = rv.prune_ops([])
    assert len(out) == 0 and len(old) == 0 and info["n_kept"] == 0
    with pytest.raises(rv.ReverieError) as e:
        rv.prune_ops(ops, wc, [wc[1]], [])
    assert e.value.code == prune_ref.ARG
    with pytest.raises(ValueError):
        rv.prune_ops(ops, wc, [-1], [])


def test_block_pruned(L):
    """a block without assertions pruned against its outputs: the ports, counts and outputs stay, and the netlist linked from it
    evaluates to the same outputs"""
    import bristol_gen
    import link_cases as lc
    import reverie_amd as rv

    nl, outputs, tail, bits, total = lc.adder_chain()
    block = nl.blocks[0]
    assert block.outputs
    pruned = block.pruned()
    want = prune_ref.sweep(block.ops, block.outputs)[0]
    assert pruned.ops.tobytes() == block.ops[want].tobytes() and pruned.prune_info["n_kept"] == len(pruned.ops)
    assert (pruned.n_ports, pruned.wire_counts, pruned.outputs, pruned.on_device) == (block.n_ports, block.wire_counts, block.outputs, False)
    # half of the block's outputs: the carry chain stays, the dropped sum bits' gates go
    half = rv.Block(block.ops, block.wire_counts, outputs=block.outputs[:len(block.outputs) // 2]).pruned()
    assert len(half.ops) < len(pruned.ops) <= len(block.ops) and half.prune_info["n_dropped"] > 0
    nl.blocks[0] = pruned
    nl.set_tail(tail(total))
    values = bristol_gen.evaluate(nl.link_host()[0], bits)
    assert sum(values[o] << k for k, o in enumerate(outputs)) == total


def test_command_line_refusals(L, tmp_path, capsys):
    from reverie_amd.__main__ import main

    prog = str(tmp_path / "p.rvops")
    program([GF2.Input(0), GF2.Mul(1, 0, 0), GF2.AssertZero(0)]).tofile(prog)
    base = ["--operation", "convert", "--program-path", prog, "--program-format", "rvops", "--output-path", str(tmp_path / "o.rvops"), "--output-format",
            "rvops", "--prune"]
    for extra in (["--window-mb", "1"], ["--compact-windows"]):
        with pytest.raises(SystemExit) as e:
            main(base + extra)
        assert e.value.code == 2
        assert "--prune needs a source that is read whole" in capsys.readouterr().err
    # and without them it prunes on the host, before anything else: counts before and after on stderr
    assert main(base) == 0
    err = capsys.readouterr().err
    assert "prune: 3 ops -> 2" in err
    assert np.fromfile(str(tmp_path / "o.rvops"), OP_DTYPE).tobytes() == program([GF2.Input(0), GF2.AssertZero(0)]).tobytes()
