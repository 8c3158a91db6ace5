"""The device compiler (csrc/compile_dev.hip, RV_COMPILE_DEVICE) against the host compiler: the same Compiled field by field on
every program the device path takes, the host compiler's status and result on every program it hands back, byte-identical proofs
(and the oracle's, on mid sizes), rv_prove_ops / rv_verify_ops under the context flag, op lists in torch tensors, and bounded
device memory over compile / destroy cycles."""
import ctypes as C

import numpy as np
import pytest

import circuits
from reverie_amd.ops import GF2, Z64, B2A, program

pytestmark = pytest.mark.gpu

RV_COMPILE_WHOLE_PROVER, RV_COMPILE_KEEP_WIRES, RV_COMPILE_DEVICE = 1, 2, 4


def _L():
    from reverie_amd import _lib

    return _lib.lib()


def _ctx():
    import reverie_amd

    return reverie_amd.Context.default()


def compare(prog, wc, flags=0):
    """-> (host status, path, diff) of rv_hook_compile_compare_device"""
    path, diff = C.c_int(-1), C.c_int(-1)
    rc = _L().rv_hook_compile_compare_device(_ctx().handle, prog.ctypes.data_as(C.c_void_p), C.c_size_t(len(prog)), C.c_size_t(wc[0]),
                                             C.c_size_t(wc[1]), C.c_uint32(flags), C.byref(path), C.byref(diff))
    return rc, path.value, diff.value


def lazy_forms_pay(levels, gates):  # compile.h
    return gates > 0 and levels > 64 and gates // levels < 256 and gates < 5000000


def k1_final(prog, wc, monkeypatch):
    """True when the K = 1 compile of the program is the host compiler's final answer"""
    from reverie_amd import _lib

    info = _lib.CircuitInfo()
    with monkeypatch.context() as m:
        m.setenv("RV_LAZY_K", "1")
        assert _L().rv_hook_compile_info(prog.ctypes.data_as(C.c_void_p), C.c_size_t(len(prog)), C.c_size_t(wc[0]), C.c_size_t(wc[1]),
                                         C.c_uint32(0), C.c_size_t(0), C.byref(info)) == 0
    gates = info.gf2_inputs + info.gf2_muls + info.gf2_asserts + info.gf2_linear
    return not lazy_forms_pay(info.levels, gates)


def edge_program():
    """wire reuse, Add(x, x), Sub of a constant, MulConst 0 / 1, Const, dead XORs, AssertZero, Random, never-written wires"""
    ops = [GF2.Input(0), GF2.Input(1), GF2.Input(2), GF2.Random(3)]
    ops += [GF2.Add(4, 0, 0), GF2.Add(5, 0, 1), GF2.Add(5, 5, 2), GF2.MulConst(6, 5, 0), GF2.MulConst(7, 5, 1), GF2.Const(8, 1),
            GF2.Add(9, 7, 8), GF2.Sub(10, 9, 11), GF2.Mul(12, 10, 3), GF2.Mul(13, 4, 12), GF2.Add(14, 12, 13), GF2.Add(15, 1, 2),
            GF2.AddConst(16, 14, 1), GF2.SubConst(16, 16, 1), GF2.Mul(0, 16, 0), GF2.Add(17, 0, 3), GF2.Add(1, 1, 1),
            GF2.AssertZero(4), GF2.AssertZero(1), GF2.Mul(18, 8, 8), GF2.Mul(19, 11, 6), GF2.Add(20, 17, 19), GF2.AssertZero(6)]
    return program(ops), (0, 24)


def random_programs():
    rng = np.random.default_rng(0xC0DE)
    progs = []
    for k in range(240):
        n_wires = int(rng.choice([3, 6, 12, 40, 150, 600]))
        n_gates = int(rng.choice([20, 120, 400, 1500, 4000]))
        prog, wit, wc = circuits.random_gf2(rng, n_in=int(rng.integers(1, 24)), n_gates=n_gates, n_wires=n_wires)
        progs.append((prog, wit, wc))
    return progs


def test_random_programs_identical(monkeypatch):
    n_dev = 0
    progs = random_programs()
    for k, (prog, wit, wc) in enumerate(progs):
        rc, path, diff = compare(prog, wc)
        assert rc == 0, k
        assert diff == 0, (k, diff)
        want = k1_final(prog, wc, monkeypatch)
        assert path == (1 if want else 0), (k, path, want)
        n_dev += path
    assert n_dev >= 200, n_dev
    prog, wc = edge_program()
    assert compare(prog, wc) == (0, 1, 0)


@pytest.mark.parametrize("recycle", [False, True])
@pytest.mark.parametrize("p_and", [0.5, 1.0])
def test_layered_mid_identical(recycle, p_and):
    prog, wit, wc, _ = circuits.layered_gf2(n_in=512, width=8192, layers=24, p_and=p_and, fold_to=128, recycle=recycle)
    assert compare(prog, wc) == (0, 1, 0)


def test_config4_full_size_identical():
    prog, wit, wc, st = circuits.layered_gf2()
    assert compare(prog, wc) == (0, 1, 0)
    aprog, _, awc, _ = circuits.layered_gf2(p_and=1.0)
    assert compare(aprog, awc) == (0, 1, 0)


def _compile_status(prog, wc, flags):
    import reverie_amd

    try:
        c = reverie_amd.Circuit(prog, wc, device_compile=bool(flags & RV_COMPILE_DEVICE), keep_wires=bool(flags & RV_COMPILE_KEEP_WIRES))
    except reverie_amd.ReverieError as e:
        return e.code, None
    info = c.info
    c.close()
    return 0, {k: v for k, v in info.items() if k not in ("compile_us", "upload_us")}


def test_fallbacks_match_host():
    z64 = program([Z64.Input(0), Z64.Input(1), Z64.Mul(2, 0, 1), GF2.Input(0)])
    b2a = program([GF2.Input(i) for i in range(64)] + [B2A(0, 0), Z64.AddConst(1, 0, 5)])
    oob = program([GF2.Input(0), GF2.Add(1, 0, 7)])
    bad = program([GF2.Input(0), GF2.Add(1, 0, 0)])
    bad["opcode"][1] = 42
    cases = [(z64, (3, 1)), (b2a, (2, 64)), (oob, (0, 4)), (bad, (0, 4))]
    for prog, wc in cases:
        rc, path, diff = compare(prog, wc)
        assert path == 0 and diff == 0
        want = _compile_status(prog, wc, 0)
        assert rc == want[0]
        assert _compile_status(prog, wc, RV_COMPILE_DEVICE) == want
    assert compare(oob, (0, 4))[0] == 3 and compare(bad, (0, 4))[0] == 5
    # KEEP_WIRES and the WHOLE_PROVER hint are the host compiler's
    prog, wit, wc, _ = circuits.layered_gf2(n_in=256, width=2048, layers=8, fold_to=128)
    assert compare(prog, wc, RV_COMPILE_KEEP_WIRES) == (0, 0, 0)
    assert compare(prog, wc, RV_COMPILE_WHOLE_PROVER) == (0, 0, 0)
    assert _compile_status(prog, wc, RV_COMPILE_KEEP_WIRES | RV_COMPILE_DEVICE) == _compile_status(prog, wc, RV_COMPILE_KEEP_WIRES)


def test_bristol_lazy_fallback():
    import bristol_gen
    from reverie_amd import bristol

    for text in (bristol_gen.aes128(), bristol_gen.sha256_block()):
        prog, info = bristol.parse(text)
        wc = info["wire_counts"]
        assert compare(prog, wc) == (0, 0, 0)
        assert _compile_status(prog, wc, RV_COMPILE_DEVICE) == _compile_status(prog, wc, 0)


def test_proofs_identical_and_oracle(oracle, rule_seeds):
    import reverie_amd

    progs = [edge_program() + (None,)]
    progs[0] = (progs[0][0], [1, 0, 1], progs[0][1])
    rng = np.random.default_rng(7)
    for _ in range(3):
        prog, wit, wc = circuits.random_gf2(rng, n_in=10, n_gates=800, n_wires=30)
        progs.append((prog, wit, wc))
    for layers, recycle in ((6, False), (10, True)):
        prog, wit, wc, _ = circuits.layered_gf2(n_in=256, width=1024, layers=layers, fold_to=128, recycle=recycle)
        progs.append((prog, list(wit), wc))
    for k, (prog, wit, wc) in enumerate(progs):
        assert compare(prog, wc)[1:] == (1, 0), k
        host = reverie_amd.Circuit(prog, wc)
        dev = reverie_amd.Circuit(prog, wc, device_compile=True)
        ph = bytes(reverie_amd.Proof.new(host, wit, [], seeds=rule_seeds))
        pd = reverie_amd.Proof.new(dev, wit, [], seeds=rule_seeds)
        assert bytes(pd) == ph, k
        assert pd.verify(dev, strict=True) and pd.verify(host, strict=True)
        if k >= len(progs) - 3:
            assert bytes(pd) == oracle.prove(prog, wit, [], wc, rule_seeds), k


def test_prove_ops_under_context_flag(rule_seeds):
    import reverie_amd

    prog, wit, wc, _ = circuits.layered_gf2(n_in=512, width=4096, layers=12, fold_to=128)
    wit = list(wit)
    plain = reverie_amd.Context(0)
    flagged = reverie_amd.Context(0)
    flagged.set_compile_flags(RV_COMPILE_DEVICE)
    want = bytes(reverie_amd.Proof.new(prog, wit, [], wc, seeds=rule_seeds, ctx=plain))
    for _ in range(2):  # cold, then from the ops cache
        got = reverie_amd.Proof.new(prog, wit, [], wc, seeds=rule_seeds, ctx=flagged)
        assert bytes(got) == want
        assert got.verify(prog, wc, ctx=flagged, strict=True)
    with pytest.raises(reverie_amd.ReverieError):
        flagged.set_compile_flags(RV_COMPILE_WHOLE_PROVER)
    flagged.set_compile_flags(0)
    assert bytes(reverie_amd.Proof.new(prog, wit, [], wc, seeds=rule_seeds, ctx=flagged)) == want
    plain.close()
    flagged.close()


def test_torch_tensor_ops(rule_seeds):
    import torch

    import reverie_amd

    prog, wit, wc, _ = circuits.layered_gf2(n_in=256, width=2048, layers=10, fold_to=128, recycle=True)
    wit = list(wit)
    host = reverie_amd.Circuit(prog, wc)
    want_info = {k: v for k, v in host.info.items() if k not in ("compile_us", "upload_us")}
    want = bytes(reverie_amd.Proof.new(host, wit, [], seeds=rule_seeds))
    raw = torch.from_numpy(prog.view(np.uint8).reshape(len(prog), 24).copy())
    for t in (raw.cuda(), raw.reshape(-1).cuda(), raw.view(torch.int64).cuda()):
        dev = reverie_amd.Circuit.from_device_ops(t, wc)
        assert {k: v for k, v in dev.info.items() if k not in ("compile_us", "upload_us")} == want_info
        assert bytes(reverie_amd.Proof.new(dev, wit, [], seeds=rule_seeds)) == want
        dev.close()
    with pytest.raises(ValueError):
        reverie_amd.Circuit.from_device_ops(raw.cuda()[:, :20], wc)
    with pytest.raises(ValueError):
        reverie_amd.Circuit.from_device_ops(raw.cuda().t(), wc)
    with pytest.raises(ValueError):
        reverie_amd.Circuit.from_device_ops(raw.cuda().float(), wc)
    # a program the device path hands back is downloaded and compiled on the host
    z = program([Z64.Input(0), Z64.Input(1), Z64.Mul(2, 0, 1), GF2.Input(0), GF2.Mul(1, 0, 0)])
    zt = torch.from_numpy(z.view(np.uint8).copy()).cuda()
    dz = reverie_amd.Circuit.from_device_ops(zt, (3, 2))
    hz = reverie_amd.Circuit(z, (3, 2))
    assert bytes(reverie_amd.Proof.new(dz, [1], [3, 5], seeds=rule_seeds)) == bytes(reverie_amd.Proof.new(hz, [1], [3, 5], seeds=rule_seeds))
    bad = torch.from_numpy(program([GF2.Input(0), GF2.Add(1, 0, 9)]).view(np.uint8).copy()).cuda()
    with pytest.raises(reverie_amd.ReverieError) as e:
        reverie_amd.Circuit.from_device_ops(bad, (0, 4))
    assert e.value.code == 3


def test_compile_cycles_bounded_memory():
    import torch

    import reverie_amd

    prog, wit, wc, _ = circuits.layered_gf2(n_in=1024, width=32768, layers=16, fold_to=128)
    ctx = reverie_amd.Context(0)
    free = []
    for _ in range(5):
        c = reverie_amd.Circuit(prog, wc, ctx=ctx, device_compile=True)
        c.close()
        ctx.sync()
        free.append(torch.cuda.mem_get_info(0)[0])
    # the arena may keep what the first cycle took; later cycles reuse it
    assert max(free[1:]) - min(free[1:]) <= (64 << 20), free
    assert free[0] - min(free[1:]) <= (64 << 20), free
    ctx.close()
