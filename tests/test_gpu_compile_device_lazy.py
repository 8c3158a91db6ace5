"""The device compiler's lazy-sum form (RV_COMPILE_WHOLE_PROVER | RV_COMPILE_DEVICE, csrc/compile_dev.hip) against the host
compiler's forced lazy-sum compile: the same Compiled field by field on the corpus that test_compile_device_lazy_host.py pins, on
layered circuits and on the Bristol circuits; the host compiler's status and result on everything the device path hands back;
byte-identical proofs, evaluations and batches; the getter that tells which compiler made a circuit."""
import ctypes as C

import numpy as np
import pytest

import circuits
import lazy_corpus
from lazy_corpus import RV_COMPILE_DEVICE, RV_COMPILE_KEEP_WIRES, RV_COMPILE_WHOLE_PROVER
from reverie_amd.ops import B2A, GF2, OP_RANDOM, Z64, program

pytestmark = pytest.mark.gpu

BOTH = RV_COMPILE_WHOLE_PROVER | RV_COMPILE_DEVICE


def _L():
    from reverie_amd import _lib

    return _lib.lib()


def _ctx():
    import reverie_amd

    return reverie_amd.Context.default()


def compare(prog, wc, flags=BOTH):
    """-> (host status, path, diff) of rv_hook_compile_compare_device"""
    path, diff = C.c_int(-1), C.c_int(-1)
    rc = _L().rv_hook_compile_compare_device(_ctx().handle, prog.ctypes.data_as(C.c_void_p), C.c_size_t(len(prog)), C.c_size_t(wc[0]),
                                             C.c_size_t(wc[1]), C.c_uint32(flags), C.byref(path), C.byref(diff))
    return rc, path.value, diff.value


def _info(c):
    return {k: v for k, v in c.info.items() if k not in ("compile_us", "upload_us")}


def test_corpus_identical():
    for k, (prog, wit, wc) in enumerate(lazy_corpus.random_programs()):
        assert compare(prog, wc) == (0, 1, 0), k


def test_crafted_program_identical():
    prog, wit, wc = lazy_corpus.crafted_program()
    diff = C.c_int(-1)  # the expectation is stable: the two host compilers agree on it
    assert _L().rv_hook_compile_compare(prog.ctypes.data_as(C.c_void_p), C.c_size_t(len(prog)), C.c_size_t(wc[0]), C.c_size_t(wc[1]),
                                        C.c_uint32(RV_COMPILE_WHOLE_PROVER), C.c_int(2), C.byref(diff)) == 0
    assert diff.value == 0
    assert compare(prog, wc) == (0, 1, 0)
    assert compare(prog, wc, 0) == (0, 1, 0)  # (and the plain form as before)


@pytest.mark.parametrize("recycle", [False, True])
@pytest.mark.parametrize("p_and", [0.5, 1.0])
def test_layered_mid_identical(recycle, p_and):
    prog, wit, wc, _ = circuits.layered_gf2(n_in=512, width=8192, layers=24, p_and=p_and, fold_to=128, recycle=recycle)
    assert compare(prog, wc) == (0, 1, 0)


@pytest.mark.parametrize("width", [63, 64, 65])
def test_small_wide_class_buckets(width):
    """a few dozen gates per level around the 64-gate step: (level, class) buckets of size 0 and 1 at the level-range bounds"""
    prog, wit, wc, _ = circuits.layered_gf2(n_in=16, width=width, layers=4, fold_to=width)
    assert compare(prog, wc) == (0, 1, 0)
    prog, wit, wc, _ = circuits.layered_gf2(n_in=16, width=width, layers=4, fold_to=width, p_and=0.9, seed=width)
    assert compare(prog, wc) == (0, 1, 0)


def test_config4_full_size_identical_lazy():
    prog, wit, wc, st = circuits.layered_gf2()
    assert compare(prog, wc) == (0, 1, 0)
    aprog, _, awc, _ = circuits.layered_gf2(p_and=1.0)
    assert compare(aprog, awc) == (0, 1, 0)


def test_bristol_forced_form_is_final():
    import bristol_gen
    from reverie_amd import bristol

    for text in (bristol_gen.aes128(), bristol_gen.sha256_block()):
        prog, info = bristol.parse(text)
        wc = info["wire_counts"]
        assert compare(prog, wc) == (0, 1, 0)
        assert compare(prog, wc, RV_COMPILE_DEVICE) == (0, 0, 0)  # (alone: the host compiler's deep-narrow recompile, as before)


def _compile_status(prog, wc, flags):
    import reverie_amd

    try:
        c = reverie_amd.Circuit(prog, wc, device_compile=bool(flags & RV_COMPILE_DEVICE), keep_wires=bool(flags & RV_COMPILE_KEEP_WIRES),
                                whole_prover=bool(flags & RV_COMPILE_WHOLE_PROVER))
    except reverie_amd.ReverieError as e:
        return e.code, None, None
    info, on = _info(c), c.compiled_on_device
    c.close()
    return 0, info, on


def test_fallbacks_match_host(monkeypatch):
    z64 = program([Z64.Input(0), Z64.Input(1), Z64.Mul(2, 0, 1), GF2.Input(0)])
    b2a = program([GF2.Input(i) for i in range(64)] + [B2A(0, 0), Z64.AddConst(1, 0, 5)])
    oob = program([GF2.Input(0), GF2.Add(1, 0, 7)])
    bad = program([GF2.Input(0), GF2.Add(1, 0, 0)])
    bad["opcode"][1] = 42
    for prog, wc in [(z64, (3, 1)), (b2a, (2, 64)), (oob, (0, 4)), (bad, (0, 4))]:
        rc, path, diff = compare(prog, wc)
        assert path == 0 and diff == 0
        want = _compile_status(prog, wc, RV_COMPILE_WHOLE_PROVER)
        assert rc == want[0]
        assert _compile_status(prog, wc, BOTH) == want  # (the host's result, and compiled_on_device False)
    assert compare(oob, (0, 4))[0] == 3 and compare(bad, (0, 4))[0] == 5
    prog, wit, wc, _ = circuits.layered_gf2(n_in=256, width=2048, layers=8, fold_to=128)
    assert compare(prog, wc, BOTH | RV_COMPILE_KEEP_WIRES) == (0, 0, 0)
    assert _compile_status(prog, wc, BOTH | RV_COMPILE_KEEP_WIRES) == _compile_status(prog, wc, RV_COMPILE_WHOLE_PROVER | RV_COMPILE_KEEP_WIRES)
    assert compare(prog, wc, RV_COMPILE_WHOLE_PROVER) == (0, 0, 0)  # (the hint alone stays a host compile)
    assert _compile_status(prog, wc, BOTH)[2] is True
    with monkeypatch.context() as m:  # RV_LAZY_K is the host compiler's
        m.setenv("RV_LAZY_K", "2")
        assert compare(prog, wc) == (0, 0, 0)
        want = _compile_status(prog, wc, RV_COMPILE_WHOLE_PROVER)
        assert _compile_status(prog, wc, BOTH) == want and want[2] is False


def test_proofs_identical_and_oracle(oracle, rule_seeds):
    import reverie_amd

    progs = [lazy_corpus.crafted_program()]
    progs += [p for p in lazy_corpus.random_programs() if 400 <= len(p[0]) <= 2000][:3]
    for layers, recycle in ((6, False), (10, True)):
        prog, wit, wc, _ = circuits.layered_gf2(n_in=256, width=1024, layers=layers, fold_to=128, recycle=recycle)
        progs.append((prog, list(wit), wc))
    assert len(progs) == 6
    seeds3 = np.stack([np.roll(np.asarray(rule_seeds, np.uint8).reshape(256, 16), b, axis=0) for b in range(3)])
    for k, (prog, wit, wc) in enumerate(progs):
        host = reverie_amd.Circuit(prog, wc, whole_prover=True)
        dev = reverie_amd.Circuit(prog, wc, whole_prover=True, device_compile=True)
        assert host.compiled_on_device is False and dev.compiled_on_device is True, k
        assert _info(dev) == _info(host), k
        ph = bytes(reverie_amd.Proof.new(host, wit, [], seeds=rule_seeds))
        pd = reverie_amd.Proof.new(dev, wit, [], seeds=rule_seeds)
        assert bytes(pd) == ph, k
        assert pd.verify(dev, strict=True) and pd.verify(host, strict=True)
        assert reverie_amd.Proof(ph).verify(dev, strict=True) and reverie_amd.Proof(ph).verify(host, strict=True)
        if k >= len(progs) - 2:
            assert bytes(pd) == oracle.prove(prog, wit, [], wc, rule_seeds), k
        if (prog["opcode"] == OP_RANDOM).any():  # (a Random wire has no cleartext value: rv_evaluate declines either circuit alike)
            for c in (host, dev):
                with pytest.raises(reverie_amd.ReverieError) as e:
                    c.evaluate(wit)
                assert e.value.code == 8
        else:
            eh, ed = host.evaluate(wit), dev.evaluate(wit)
            assert (ed.ok, ed.n_failed, ed.first_failed_op) == (eh.ok, eh.n_failed, eh.first_failed_op) and ed.ok, k
        wits = np.tile(np.asarray(wit, np.uint8), (3, 1))
        bh = reverie_amd.Proof.new_batch(host, wits, seeds=seeds3)
        bd = reverie_amd.Proof.new_batch(dev, wits, seeds=seeds3)
        assert [bytes(p) for p in bd] == [bytes(p) for p in bh], k
        assert bytes(bd[0]) == ph, k
        host.close()
        dev.close()


def test_torch_tensor_ops(rule_seeds):
    import torch

    import reverie_amd

    prog, wit, wc, _ = circuits.layered_gf2(n_in=256, width=2048, layers=10, fold_to=128, recycle=True)
    wit = list(wit)
    host = reverie_amd.Circuit(prog, wc, whole_prover=True)
    want = bytes(reverie_amd.Proof.new(host, wit, [], seeds=rule_seeds))
    t = torch.from_numpy(prog.view(np.uint8).reshape(len(prog), 24).copy()).cuda()
    dev = reverie_amd.Circuit.from_device_ops(t, wc, whole_prover=True)
    assert dev.compiled_on_device is True and host.compiled_on_device is False
    assert _info(dev) == _info(host)
    assert bytes(reverie_amd.Proof.new(dev, wit, [], seeds=rule_seeds)) == want
    plain = reverie_amd.Circuit.from_device_ops(t, wc)
    assert plain.compiled_on_device is True and plain.info["gf2_linear"] > dev.info["gf2_linear"]
    for c in (host, dev, plain):
        c.close()


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
    with pytest.raises(reverie_amd.ReverieError):
        flagged.set_compile_flags(BOTH)
    plain.close()
    flagged.close()


def test_compile_cycles_bounded_memory():
    import torch

    import reverie_amd

    prog, wit, wc, _ = circuits.layered_gf2(n_in=1024, width=32768, layers=16, fold_to=128)
    ctx = reverie_amd.Context(0)
    free = []
    for _ in range(5):
        c = reverie_amd.Circuit(prog, wc, ctx=ctx, whole_prover=True, device_compile=True)
        assert c.compiled_on_device
        c.close()
        ctx.sync()
        free.append(torch.cuda.mem_get_info(0)[0])
    # the arena may keep what the first cycle took; later cycles reuse it
    assert max(free[1:]) - min(free[1:]) <= (64 << 20), free
    assert free[0] - min(free[1:]) <= (64 << 20), free
    ctx.close()
