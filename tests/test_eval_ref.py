"""The batched cleartext reference (tests/eval_ref.py) pinned on the host: against model() of test_gpu_eval.py, the oracle's
prover-side wire values, bristol_gen.evaluate, and its own layer-by-layer variant.  No GPU."""
import numpy as np
import pytest

import bristol_gen
import circuits
import eval_ref
from reverie_amd import bristol
from test_gpu_eval import ONE, ZERO8, model, random_program


def _witnesses(rng, B, n2=10, n64=4, mixed=True):
    w2 = rng.integers(0, 2, (B, n2)).astype(np.uint8)
    w64 = rng.integers(0, 1 << 64, (B, n64), dtype=np.uint64) if mixed else np.zeros((B, 0), np.uint64)
    return w2, w64


@pytest.mark.parametrize("mixed", [False, True])
def test_agrees_with_model_per_witness(mixed):
    rng = np.random.default_rng(21 + mixed)
    seen_fail = seen_ok = False
    for trial in range(10):
        prog, wc = random_program(rng, n_gates=400, mixed=mixed, p_assert=0.04 if trial % 2 else 0.0)
        B = 37
        w2, w64 = _witnesses(rng, B, mixed=mixed)
        w2[::5] *= 0xFF  # (non-zero bytes other than 1 count as 1)
        g, z, nf, ff = eval_ref.evaluate(prog, wc, w2, w64)
        assert g.shape == (B, wc[1]) and z.shape == (B, wc[0])
        for k in range(B):
            mg, mz, fails = model(prog, wc, w2[k], w64[k])
            assert np.array_equal(g[k], mg) and np.array_equal(z[k], mz), (trial, k)
            assert nf[k] == len(fails) and ff[k] == (fails[0] if fails else -1), (trial, k)
            seen_fail |= bool(fails)
            seen_ok |= not fails
    assert seen_fail and seen_ok


@pytest.mark.parametrize("mixed", [False, True])
def test_agrees_with_oracle_wire_values(oracle, mixed):
    rng = np.random.default_rng(31 + mixed)
    for trial in range(6):
        prog, wc = random_program(rng, n_gates=250, mixed=mixed, p_assert=0.0)
        w2, w64 = _witnesses(rng, 3, mixed=mixed)
        g, z, nf, _ = eval_ref.evaluate(prog, wc, w2, w64)
        assert not nf.any()
        for k in range(3):
            for w in rng.choice(wc[1], 3, replace=False):
                og, _ = oracle.group_wire_values(prog, w2[k], w64[k], wc, ZERO8, gf2_wire=int(w))
                assert og == (ONE if g[k, w] else 0), (trial, k, w)
            for w in (rng.choice(wc[0], 3, replace=False) if mixed else []):
                _, oz = oracle.group_wire_values(prog, w2[k], w64[k], wc, ZERO8, z64_wire=int(w))
                assert all(int(x) == int(z[k, w]) for x in oz), (trial, k, w)


def test_agrees_with_bristol_adder():
    prog, info = bristol.parse(bristol_gen.adder64())
    rng = np.random.default_rng(2)
    w2 = rng.integers(0, 2, (20, 128)).astype(np.uint8)
    g, _, nf, _ = eval_ref.evaluate(prog, info["wire_counts"], w2)
    assert not nf.any()
    for k in range(20):
        v = bristol_gen.evaluate(prog, w2[k].tolist())
        assert g[k, :len(v)].tolist() == v[:info["wire_counts"][1]]
        x = sum(int(w2[k, i]) << i for i in range(64))
        y = sum(int(w2[k, 64 + i]) << i for i in range(64))
        out = g[k, info["n_wires"] - 64:info["n_wires"]]
        assert sum(int(o) << i for i, o in enumerate(out)) == (x + y) % (1 << 64)


def _same(r1, r2):
    return all(np.array_equal(x, y) for x, y in zip(r1, r2))


@pytest.mark.parametrize("B", [1, 63, 65, 130])
def test_layers_agree_with_generic(B):
    rng = np.random.default_rng(B)
    prog, wit, wc, _ = circuits.layered_gf2(n_in=64, width=512, layers=5, fold_to=16)
    w2 = np.tile(np.asarray(wit, np.uint8), (B, 1))
    w2[1:] = rng.integers(0, 3, w2[1:].shape)  # (witness 0 satisfies every assertion; the others mostly fail some)
    ls = eval_ref.layers(prog)
    assert len(ls) >= 5 + 4 + 16  # inputs, 5 layers, the fold, AddConst / AssertZero pairs
    r = eval_ref.evaluate_layers(prog, wc, w2, bounds=ls)
    assert _same(r, eval_ref.evaluate(prog, wc, w2))
    assert r[2][0] == 0 and (B == 1 or r[2].any())
    prog, wit, wc, _ = circuits.layered_z64(n_in=64, width=256, n_mul=600, fold_to=8)
    w64 = np.tile(np.asarray(wit, np.uint64), (B, 1))
    w64[1:] = rng.integers(0, 1 << 64, w64[1:].shape, dtype=np.uint64)
    r = eval_ref.evaluate_layers(prog, wc, None, w64)
    assert _same(r, eval_ref.evaluate(prog, wc, None, w64))
    assert r[2][0] == 0 and (B == 1 or r[2][1:].all())
    # a random program: recycled wires, every op kind, layers of one or two ops
    prog, wc = random_program(rng, n_gates=600, mixed=False, p_assert=0.05)
    w2 = rng.integers(0, 2, (B, 10)).astype(np.uint8)
    assert _same(eval_ref.evaluate_layers(prog, wc, w2), eval_ref.evaluate(prog, wc, w2))


def test_layers_refuse_b2a():
    prog, wc = random_program(np.random.default_rng(0), n_gates=400, mixed=True)
    with pytest.raises(ValueError, match="B2A"):
        eval_ref.layers(prog)
