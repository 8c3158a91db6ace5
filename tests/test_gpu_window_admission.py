"""The admission rule of the windowed stages (csrc/win_pass.inc), which rv_compactor_*, rv_pruner_* and rv_folder_*
share: a call out of order is RV_E_ARG whatever its pointers are, and moves nothing.  Each stage gets a call that is out of order AND
carries a misaligned device pointer; it has to answer RV_E_ARG on the host, leave get_info() as it was, and then run its passes to
the whole-list call's bytes."""
import ctypes as C

import numpy as np
import pytest

from reverie_amd.ops import GF2, OP_DTYPE, program

pytestmark = pytest.mark.gpu

ARG = 9
OP_BYTES = OP_DTYPE.itemsize
N = 64
WC = (0, N)  # (z64, gf2): SSA, the op's ordinal is its wire
OUTPUTS = (40, 50)
CUTTINGS = {"one_feed": [(0, N)], "1_62_1": [(0, 1), (1, N - 1), (N - 1, N)]}


def make_list():
    """64 GF(2) ops: Inputs, two Consts (something to fold), Adds and Muls of earlier wires (some dead: something to prune), an
    AssertZero at the end"""
    rng = np.random.default_rng(64)
    ops = [GF2.Input(i) for i in range(6)] + [GF2.Const(6, 1), GF2.Const(7, 0)]
    for i in range(8, N - 1):
        a, b = (int(x) for x in rng.integers(0, i, 2))
        ops.append(GF2.Mul(i, a, b) if i % 3 == 0 else GF2.Add(i, a, b))
    ops.append(GF2.AssertZero(N - 2))
    assert len(ops) == N
    return program(ops)


OPS = make_list()


@pytest.fixture(scope="module")
def rv():
    import reverie_amd

    reverie_amd.Context.default()
    return reverie_amd


@pytest.fixture(scope="module")
def src(rv):
    """the list in device memory with room behind it, so that a pointer 4 bytes on still lies inside the tensor"""
    import torch

    t = torch.zeros(((N + 1) * OP_BYTES,), dtype=torch.uint8, device="cuda")
    t[:N * OP_BYTES] = torch.from_numpy(OPS.view(np.uint8).copy()).cuda()
    torch.cuda.synchronize()
    return t


@pytest.fixture(scope="module")
def whole(rv):
    """the whole-list calls' results, computed once"""
    return {"compact": rv.compact_wires(OPS, WC)[0].tobytes(), "prune": rv.prune_ops(OPS, WC, OUTPUTS)[0].tobytes(),
            "fold": rv.fold_ops(OPS, WC)[0].tobytes()}


def feeds(src, cutting):
    recs = src[:N * OP_BYTES].reshape(N, OP_BYTES)
    return [recs[lo:hi] for lo, hi in CUTTINGS[cutting]]


def room():
    import torch

    return torch.full((N * OP_BYTES,), 0xA5, dtype=torch.uint8, device="cuda")


def as_bytes(tensors):
    return b"".join(t.cpu().numpy().tobytes() for t in tensors)


@pytest.mark.parametrize("cutting", list(CUTTINGS))
def test_compactor_feed_before_scan_end(rv, src, whole, cutting):
    from reverie_amd import _lib

    with rv.compact.DeviceCompactor(WC) as dc:
        for f in feeds(src, cutting):
            dc.scan(f)
        before, out = dc.get_info(), room()
        assert _lib.lib().rv_compactor_feed(dc.handle, C.c_void_p(src.data_ptr() + 4), C.c_size_t(N), 1, C.c_void_p(out.data_ptr())) == ARG
        assert dc.get_info() == before and as_bytes([out]) == b"\xA5" * (N * OP_BYTES)
        assert dc.scan_end() is False
        assert as_bytes([dc.feed(f) for f in feeds(src, cutting)]) == whole["compact"]


@pytest.mark.parametrize("cutting", list(CUTTINGS))
def test_pruner_feed_before_scan_end(rv, src, whole, cutting):
    from reverie_amd import _lib

    with rv.prune.DevicePruner(WC, OUTPUTS) as dp:
        for f in feeds(src, cutting):
            dp.scan(f)
        before, out, n_out = dp.get_info(), room(), C.c_size_t(0)
        assert _lib.lib().rv_pruner_feed(dp.handle, C.c_void_p(src.data_ptr() + 4), C.c_size_t(N), 1, C.c_void_p(out.data_ptr()), C.c_size_t(N),
                                         C.byref(n_out), None) == ARG
        assert dp.get_info() == before and as_bytes([out]) == b"\xA5" * (N * OP_BYTES)
        dp.scan_end()
        for f in reversed(feeds(src, cutting)):
            dp.mark(f)
        dp.mark_end()
        assert as_bytes([dp.feed(f)[0] for f in feeds(src, cutting)]) == whole["prune"]


@pytest.mark.parametrize("cutting", list(CUTTINGS))
def test_folder_replay_before_end(rv, src, whole, cutting):
    from reverie_amd import _lib

    with rv.fold.DeviceFolder(WC, keep_log=True) as df:
        folded = [df.feed(f) for f in feeds(src, cutting)]
        before, out = df.get_info(), room()
        assert _lib.lib().rv_folder_replay(df.handle, C.c_void_p(src.data_ptr() + 4), C.c_size_t(N), 1, C.c_uint64(0), C.c_void_p(out.data_ptr())) == ARG
        assert df.get_info() == before and as_bytes([out]) == b"\xA5" * (N * OP_BYTES)
        df.end()
        assert as_bytes(folded) == whole["fold"]
        assert as_bytes([df.replay(f, lo) for f, (lo, _) in zip(feeds(src, cutting), CUTTINGS[cutting])]) == whole["fold"]
        df.replay_end()
