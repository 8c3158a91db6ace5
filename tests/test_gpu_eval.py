"""Cleartext evaluation on the GPU (rv_evaluate / rv_evaluate_batch): values against a numpy model and the oracle, verdicts
against the prover, batches, known answers, the proofs of keep_wires circuits, errors, the CLI."""
import ctypes as C
import hashlib
import os

import numpy as np
import pytest

import bristol_gen
import circuits
import eval_ref
from conftest import golden_matches
from reverie_amd.ops import B2A, GF2, OP_DTYPE, Z64, SizeHint, program

pytestmark = pytest.mark.gpu

M64 = (1 << 64) - 1
ONE = 0xFFFFFFFFFFFFFFFF
ZERO8 = np.zeros((8, 16), np.uint8)


@pytest.fixture(scope="module")
def rv():
    import reverie_amd

    reverie_amd.Context.default()
    return reverie_amd


def schedules():
    from reverie_amd import _lib

    out = (C.c_uint64 * 2)()
    assert _lib.lib().rv_hook_eval_schedules(out) == 0
    return int(out[0]), int(out[1])


# ---------------------------------------------------------------- programs and the model
def random_program(rng, n_gates=300, mixed=True, p_assert=0.04):
    """Random-free program over both domains (or GF(2) only): recycled wires, B2A bridges, a SizeHint, asserts on arbitrary
    wires (so that some witnesses fail them), wires never written"""
    n2, n64 = 100, 12
    ops = [SizeHint(n64, n2)] + [GF2.Input(i) for i in range(10)] + ([Z64.Input(i) for i in range(4)] if mixed else [])
    kinds = ["mul2", "add2", "sub2", "addc2", "mulc2", "const2", "assert2"]
    p = [0.3, 0.25, 0.05, 0.1, 0.05, 0.05, p_assert]
    if mixed:
        kinds += ["mul64", "add64", "sub64", "mulc64", "addc64", "subc64", "const64", "b2a", "assert64"]
        p += [0.1, 0.06, 0.04, 0.03, 0.03, 0.02, 0.02, 0.04, p_assert / 2]
    p = np.asarray(p) / sum(p)
    for _ in range(n_gates):
        k = kinds[rng.choice(len(kinds), p=p)]
        d, a, b = (int(x) for x in rng.integers(0, 30, 3))
        c = int(rng.integers(0, 1 << 63, dtype=np.uint64)) * 2 + 1
        if k.endswith("64"):
            d, a, b = d % n64, a % n64, b % n64
        op = {"mul2": lambda: GF2.Mul(d, a, b), "add2": lambda: GF2.Add(d, a, b), "sub2": lambda: GF2.Sub(d, a, b),
              "addc2": lambda: GF2.AddConst(d, a, 1), "mulc2": lambda: GF2.MulConst(d, a, (c >> 1) & 1), "const2": lambda: GF2.Const(d, 1),
              "assert2": lambda: GF2.AssertZero(a), "mul64": lambda: Z64.Mul(d, a, b), "add64": lambda: Z64.Add(d, a, b),
              "sub64": lambda: Z64.Sub(d, a, b), "mulc64": lambda: Z64.MulConst(d, a, c), "addc64": lambda: Z64.AddConst(d, a, c),
              "subc64": lambda: Z64.SubConst(d, a, c), "const64": lambda: Z64.Const(d, c), "b2a": lambda: B2A(d % n64, a % 6),
              "assert64": lambda: Z64.AssertZero(a)}[k]()
        ops.append(op)
    return program(ops), (n64, n2)


def model(prog, wc, w2, w64):
    """(gf2 values, z64 values, op indices of the failing AssertZero ops) -- the clear semantics of interpreter/single.rs and
    combine.rs, written out"""
    n64, n2 = wc
    v2, v64 = [0] * n2, [0] * n64
    i2 = i64 = 0
    fails = []
    for i, (dom, opc, _r, d, a, b, imm) in enumerate(prog.tolist()):
        if dom == 3:
            v2 += [0] * max(0, b - len(v2))
            v64 += [0] * max(0, a - len(v64))
            continue
        if dom == 2:
            v64[d] = sum(v2[a + k] << k for k in range(64))
            continue
        v = v2 if dom == 0 else v64
        if opc == 0:
            if dom == 0:
                v[d] = int(w2[i2]) & 1 if w2[i2] in (0, 1) else int(bool(w2[i2]))
                i2 += 1
            else:
                v[d] = int(w64[i64])
                i64 += 1
        elif opc == 8:
            if v[a]:
                fails.append(i)
        elif dom == 0:
            v[d] = {2: lambda: v[a] ^ v[b], 4: lambda: v[a] ^ v[b], 3: lambda: v[a] ^ (imm & 1), 5: lambda: v[a] ^ (imm & 1),
                    6: lambda: v[a] & v[b], 7: lambda: v[a] & (imm & 1), 9: lambda: imm & 1}[opc]()
        else:
            v[d] = {2: lambda: v[a] + v[b], 4: lambda: v[a] - v[b], 3: lambda: v[a] + imm, 5: lambda: v[a] - imm,
                    6: lambda: v[a] * v[b], 7: lambda: v[a] * imm, 9: lambda: imm}[opc]() & M64
    return np.array(v2[:n2], np.uint8), np.array(v64[:n64], np.uint64), fails


def witness(rng, B=None):
    shape = (10,) if B is None else (B, 10)
    return rng.integers(0, 2, shape).astype(np.uint8), rng.integers(0, 1 << 63, shape[:-1] + (4,), dtype=np.uint64)


# ---------------------------------------------------------------- 1. values: model and oracle
@pytest.mark.parametrize("mixed", [False, True])
def test_values_equal_model_and_oracle(rv, oracle, mixed):
    rng = np.random.default_rng(11 + mixed)
    n_oracle = 0
    for trial in range(12):
        prog, wc = random_program(rng, mixed=mixed, p_assert=0.04 if trial % 2 else 0.0)  # (even trials: every assertion holds)
        w2, w64 = witness(rng)
        if not mixed:
            w64 = w64[:0]
        g, z, fails = model(prog, wc, w2, w64)
        r = rv.Circuit(prog, wc, keep_wires=True).evaluate(w2, w64)
        assert np.array_equal(r.gf2, g) and np.array_equal(r.z64, z), trial
        assert r.ok == (not fails) and r.n_failed == len(fails) and r.first_failed_op == (fails[0] if fails else None)
        if fails:
            continue
        for w in rng.choice(wc[1], 4, replace=False):
            og, _ = oracle.group_wire_values(prog, w2, w64, wc, ZERO8, gf2_wire=int(w))
            assert og == (ONE if g[w] else 0), (trial, w)
        for w in range(min(wc[0], 4) if mixed else 0):
            _, oz = oracle.group_wire_values(prog, w2, w64, wc, ZERO8, z64_wire=w)
            assert all(int(x) == int(z[w]) for x in oz), (trial, w)  # (B2A: the value the prover holds)
        n_oracle += 1
    assert n_oracle >= 6


# ---------------------------------------------------------------- 2. verdicts: the prover's
def test_verdict_agrees_with_the_prover(rv, oracle):
    from reverie_amd import _lib

    rng = np.random.default_rng(5)
    seen = set()
    for trial in range(16):
        prog, wc = random_program(rng, n_gates=120, mixed=trial % 2 == 1, p_assert=0.02)
        w2, w64 = witness(rng)
        r = rv.Circuit(prog, wc).evaluate(w2, w64)
        seeds = rng.integers(0, 256, (256, 16), dtype=np.uint8)
        try:
            rv.Proof.new(prog, w2, w64, wc, seeds=seeds)
            proved = True
        except _lib.ReverieError as e:
            assert e.code == 1
            proved = False
        try:
            oracle.prove(prog, w2, w64, wc, seeds)
            oproved = True
        except oracle.OracleError as e:
            assert e.code == 1
            oproved = False
        assert r.ok == proved == oproved, trial
        _, _, fails = model(prog, wc, w2, w64)
        assert r.first_failed_op == (fails[0] if fails else None)
        seen.add(r.ok)
    assert seen == {True, False}


# ---------------------------------------------------------------- 3. batches, both schedules
def rv_bristol(text, expected=None):
    from reverie_amd import bristol

    return bristol.parse(text, expected_outputs=expected)


def _wide(seed=3):
    """wide and shallow: 3 layers of 16384 gates (one launch per level)"""
    prog, _w, wc, _st = circuits.layered_gf2(n_in=512, width=16384, layers=3, seed=seed)
    return prog, wc


@pytest.mark.parametrize("B", [1, 31, 32, 33, 1000])
def test_batches_equal_single_calls(rv, B):
    rng = np.random.default_rng(B)
    s0 = schedules()
    adder, info = rv_bristol(bristol_gen.adder64(), expected=[0] * 64)
    wide, wwc = _wide()
    cases = [(adder, info["wire_counts"], 128), (wide, wwc, 512)]
    mixed, mwc = random_program(np.random.default_rng(7), n_gates=400, mixed=True)
    cases.append((mixed, mwc, 10))
    for prog, wc, n_in in cases:
        c = rv.Circuit(prog, wc, keep_wires=True)
        w2 = rng.integers(0, 2, (B, n_in)).astype(np.uint8)
        if prog is adder:
            # a + b == 0 (mod 2^64) holds for b = -a: valid witnesses, with invalid ones planted at known indices
            a = rng.integers(0, 1 << 63, B, dtype=np.uint64)
            b = (0 - a.astype(object)) % (1 << 64)
            for k in range(B):
                w2[k, :64] = [(int(a[k]) >> i) & 1 for i in range(64)]
                w2[k, 64:] = [(int(b[k]) >> i) & 1 for i in range(64)]
            bad = sorted({0, B // 2, B - 1})
            for k in bad:
                w2[k, 64] ^= 1
        w64 = rng.integers(0, 1 << 63, (B, 4), dtype=np.uint64) if prog is mixed else None
        r = c.evaluate_batch(w2, w64, values=True)
        if prog is adder:
            assert [k for k in range(B) if not r.ok[k]] == bad
        for k in sorted(set([0, B - 1, B // 2] + list(rng.integers(0, B, 6)))):
            one = c.evaluate(w2[k], w64[k] if w64 is not None else [])
            assert bool(r.ok[k]) == one.ok and int(r.n_failed[k]) == one.n_failed
            assert (int(r.first_failed_op[k]) if r.first_failed_op[k] >= 0 else None) == one.first_failed_op
            assert np.array_equal(r.gf2[k], one.gf2) and np.array_equal(r.z64[k], one.z64)
        plain = c.evaluate_batch(w2, w64)
        assert np.array_equal(plain.ok, r.ok) and plain.gf2 is None
        # every output against the independent reference (the wide circuit layer by layer)
        g, z, nf, ff = (eval_ref.evaluate_layers if prog is wide else eval_ref.evaluate)(prog, wc, w2, w64)
        assert np.array_equal(r.n_failed, nf) and np.array_equal(r.first_failed_op, ff)
        assert np.array_equal(r.gf2, g) and np.array_equal(r.z64, z)
    s1 = schedules()
    assert s1[0] > s0[0] and s1[1] > s0[1]  # both schedules ran


# ---------------------------------------------------------------- 4. known answers
def _bits_msb(data: bytes):
    return [(byte >> (7 - k)) & 1 for byte in data for k in range(8)]


def _bytes_msb(bits):
    return bytes(int("".join(str(int(b)) for b in bits[8 * i:8 * i + 8]), 2) for i in range(len(bits) // 8))


def _outputs(rv, text, wits):
    prog, info = rv_bristol(text)
    c = rv.Circuit(prog, info["wire_counts"], keep_wires=True)
    r = c.evaluate_batch(np.asarray(wits, np.uint8), values=True)
    n_out = sum(int(x) for x in text.splitlines()[2].split()[1:])
    return r.gf2[:, info["n_wires"] - n_out:info["n_wires"]]


def test_aes128_fips197(rv):
    key, pt = bytes(range(16)), bytes.fromhex("00112233445566778899aabbccddeeff")
    out = _outputs(rv, bristol_gen.aes128(), [_bits_msb(key + pt)])
    assert _bytes_msb(out[0]).hex() == "69c4e0d86a7b0430d8cdb78070b4c55a"


def _pad(msg: bytes) -> bytes:
    return msg + b"\x80" + bytes(55 - len(msg)) + (8 * len(msg)).to_bytes(8, "big")


def test_sha256_one_block_and_batch(rv):
    text = bristol_gen.sha256_block()
    out = _outputs(rv, text, [_bits_msb(_pad(b"abc"))])
    assert _bytes_msb(out[0]) == hashlib.sha256(b"abc").digest()
    rng = np.random.default_rng(9)
    msgs = [bytes(rng.integers(0, 256, int(rng.integers(0, 56)), dtype=np.uint8)) for _ in range(70)]
    out = _outputs(rv, text, [_bits_msb(_pad(m)) for m in msgs])
    for m, o in zip(msgs, out):
        assert _bytes_msb(o) == hashlib.sha256(m).digest()


def test_adder_batch(rv):
    rng = np.random.default_rng(4)
    a = rng.integers(0, 1 << 63, 100, dtype=np.uint64) * 2 + 1
    b = rng.integers(0, 1 << 63, 100, dtype=np.uint64) * 3
    wits = [[(int(x) >> i) & 1 for i in range(64)] + [(int(y) >> i) & 1 for i in range(64)] for x, y in zip(a, b)]
    out = _outputs(rv, bristol_gen.adder64(), wits)
    for x, y, o in zip(a, b, out):
        assert sum(int(v) << i for i, v in enumerate(o)) == (int(x) + int(y)) % (1 << 64)


# ---------------------------------------------------------------- 5. the 10^7-gate benchmark circuit
def test_config4_full_size(rv, oracle):
    prog, wit, wc, _st = circuits.layered_gf2()
    c = rv.Circuit(prog, wc, keep_wires=True)
    r = c.evaluate(wit)
    assert r.ok and r.n_failed == 0 and r.first_failed_op is None
    assert c.evaluate(wit).ok  # (no wire vector)
    rng = np.random.default_rng(1)
    for w in rng.choice(wc[1], 2, replace=False):
        og, _ = oracle.group_wire_values(prog, wit, [], wc, ZERO8, gf2_wire=int(w))
        assert og == (ONE if r.gf2[w] else 0)
    g, _z, nf, _ff = eval_ref.evaluate_layers(prog, wc, wit)  # (every wire)
    assert nf[0] == 0 and np.array_equal(r.gf2, g[0])


# ---------------------------------------------------------------- 6. proofs of keep_wires circuits, errors
def test_keep_wires_proofs_are_golden(rv, oracle, rule_seeds):
    import test_gpu_parity as tp

    for name in tp.ALL_GOLDEN:
        m, prog, w2, w64, wc, _gold = tp.load_case(name)
        for whole_prover in (False, True):  # (whole_prover: lazy forms of up to RV_LIN_K rows)
            c = rv.Circuit(prog, wc, whole_prover=whole_prover, keep_wires=True)
            assert golden_matches(oracle, name, m, bytes(rv.Proof.new(c, w2, w64, seeds=rule_seeds))), (name, whole_prover)


def test_errors(rv):
    from reverie_amd import _lib

    with pytest.raises(_lib.ReverieError) as e:
        rv.Circuit(program([GF2.Input(0), GF2.Random(1), GF2.Add(2, 0, 1)]), (0, 3)).evaluate([1])
    assert e.value.code == 8
    with pytest.raises(_lib.ReverieError) as e:
        rv.Circuit(program([Z64.Random(0)]), (1, 0)).evaluate([])
    assert e.value.code == 8
    c = rv.Circuit(program([GF2.Input(0), GF2.Input(1), GF2.Mul(2, 0, 1)]), (0, 3))
    with pytest.raises(_lib.ReverieError) as e:
        c.evaluate([1])
    assert e.value.code == 2
    st = _lib.EvalStatus()
    w = np.ones(2, np.uint8)
    vals = np.zeros(3, np.uint8)
    rc = _lib.lib().rv_evaluate(c.ctx.handle, c.handle, w.ctypes.data_as(C.c_void_p), C.c_size_t(2), None, C.c_size_t(0),
                                vals.ctypes.data_as(C.c_void_p), None, C.byref(st))
    assert rc == 9  # values of a circuit compiled without RV_COMPILE_KEEP_WIRES
    assert c.evaluate([1, 1]).ok
    g, z = rv.evaluate_composite_program(program([GF2.Input(0), GF2.Input(1), GF2.Mul(2, 0, 1)]), [1, 1])
    assert g.tolist() == [1, 1, 1] and len(z) == 0
    with pytest.raises(ValueError, match="op 3"):
        rv.evaluate_composite_program(program([GF2.Input(0), GF2.Input(1), GF2.Mul(2, 0, 1), GF2.AssertZero(2)]), [1, 1])


# ---------------------------------------------------------------- 7. the CLI
def test_cli_oneshot_gpu(rv, tmp_path, capsys):
    from reverie_amd.__main__ import main

    # a mixed program (the CLI's witness is GF(2) bits: its Z64 values come from B2A and constants)
    ops = [GF2.Input(i) for i in range(64)] + [B2A(0, 0), Z64.Const(1, 5), Z64.Mul(2, 0, 1), Z64.SubConst(3, 2, 5 * 6),
                                              Z64.AssertZero(3)]
    p = tmp_path / "m.rvops"
    p.write_bytes(program(ops).tobytes())
    w = tmp_path / "w.txt"
    w.write_text("\n".join(str((6 >> i) & 1) for i in range(64)) + "\n")
    assert main(["--operation", "oneshot", "--evaluator", "gpu", "--program-path", str(p), "--witness-path", str(w)]) == 0
    assert capsys.readouterr().out.splitlines() == ["Evaluating program in cleartext", "()"]
    w.write_text("\n".join(str((7 >> i) & 1) for i in range(64)) + "\n")
    with pytest.raises(SystemExit) as e:
        main(["--operation", "oneshot", "--program-path", str(p), "--witness-path", str(w)])  # (auto: Z64 ops -> GPU)
    assert "op %d" % (len(ops) - 1) in str(e.value)
    # the adder with its expected outputs
    bp = tmp_path / "adder.txt"
    bp.write_text(bristol_gen.adder64())
    x, y = 12345, 67890
    w.write_text("\n".join(str(b) for b in [(x >> i) & 1 for i in range(64)] + [(y >> i) & 1 for i in range(64)]) + "\n")
    e_path = tmp_path / "e.txt"
    e_path.write_text("\n".join(str(((x + y) >> i) & 1) for i in range(64)) + "\n")
    args = ["--operation", "oneshot", "--evaluator", "gpu", "--program-path", str(bp), "--witness-path", str(w), "--expected-outputs-path", str(e_path)]
    assert main(args) == 0
    e_path.write_text("\n".join(str(((x + y + 1) >> i) & 1) for i in range(64)) + "\n")
    with pytest.raises(SystemExit) as e:
        main(args)
    assert "AssertZero at op" in str(e.value)
