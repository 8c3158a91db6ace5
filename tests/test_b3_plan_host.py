"""Which transcript-hash kernel production picks for which shape (b3_tree.hip: b3_choose_* / b3_plan_*, through rv_hook_b3_plan), on
both sides of every threshold.  tests/test_gpu_b3_kernels.py runs every kernel at small shapes with the choice forced; this table plus
the whole-proof tests cover "the right kernel runs".  (No GPU: the hook takes no context.)

The expectations restate the rules as the launchers' comments give them, not the code: a lane takes ONE repetition while
chunks x lanes x batch < 128 x 1024 or the quad list covers a quarter of the row or less; full rows without a list otherwise take the
chunk-per-wavefront kernel; a tree is reduced four-to-one while it has more than 512 nodes; a lane per repetition runs the top when
batch >= 8 or n <= 4; both streams of a small proof share their launches up to 64 chunks each and below 64 x 1024 lanes."""
import ctypes as C

import pytest

RPL1, RPL4, UNI = 1, 2, 3
LANE, TAIL64, TAIL512 = 1, 2, 3
PAIR_Q, PAIR_LANE = 1, 2
LANES = 128 * 1024
E_ARG = 9


@pytest.fixture(scope="module")
def plan():
    import os

    from reverie_amd import _lib

    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__

        __graft_entry__.build()
    L = _lib.lib()

    def call(c_pre=1, c_on=1, NQ=64, n_quads=None, batch=0, exact=True):
        """chunks of the two streams -> the 13 answers; exact: streams that end on a chunk boundary, else one event into the last chunk"""
        out = (C.c_uint32 * 13)()
        ev = (lambda c: c * 1024) if exact else (lambda c: (c - 1) * 1024 + 1)
        rc = L.rv_hook_b3_plan(ev(c_pre), ev(c_on), NQ, n_quads is not None, n_quads or 0, batch, out)
        assert rc == 0, rc
        return list(out)

    call.lib = L
    return call


@pytest.mark.parametrize("NQ", [64, 16])
@pytest.mark.parametrize("batch", [0, 1, 8, 256])
def test_chunk_kernel_lane_threshold(plan, NQ, batch):
    edge = LANES // (NQ * max(batch, 1))  # chunks at which chunks x NQ x batch reaches 128 x 1024
    assert edge * NQ * max(batch, 1) == LANES
    wide = UNI if NQ == 64 else RPL4
    for exact in (True, False):
        below, at = plan(edge - 1, edge - 1, NQ, batch=batch, exact=exact), plan(edge, edge, NQ, batch=batch, exact=exact)
        assert below[0] == RPL1 and below[1] == RPL1, (NQ, batch)
        assert at[0] == wide and at[1] == wide, (NQ, batch)
    assert plan(1, 1, NQ, batch=batch)[:2] == [RPL1, RPL1]
    assert plan(0, 0, NQ, batch=batch, exact=True)[:2] == [RPL1, RPL1]  # (the empty stream: one empty chunk)


@pytest.mark.parametrize("NQ", [64, 16])
def test_chunk_kernel_quad_list(plan, NQ):
    many = LANES  # chunks: far past the lane threshold whatever the list
    assert plan(1, many, NQ, n_quads=NQ // 4)[0] == RPL1       # a quarter of the row: a repetition per lane at any size
    assert plan(1, many, NQ, n_quads=NQ // 4 + 1)[0] == RPL4   # more: a quad word per lane (never the chunk-per-wavefront kernel)
    assert plan(1, many, NQ, n_quads=NQ)[0] == RPL4
    assert plan(1, many, NQ, n_quads=1)[0] == RPL1
    # with a long list the lane threshold counts the LISTED quad words
    nq = NQ // 4 + 1
    edge = -(-LANES // nq)
    assert plan(1, edge - 1, NQ, n_quads=nq)[0] == RPL1 and plan(1, edge, NQ, n_quads=nq)[0] == RPL4
    # the bit rows never see the list
    assert plan(many, 1, NQ, n_quads=1)[1] == (UNI if NQ == 64 else RPL4)


def test_empty_quad_list_launches_nothing(plan):
    for c in (1, 64, 4900):
        got = plan(c, c, 64, n_quads=0)
        assert got[0] == 0 and got[8] == 0 and got[9] == 0 and got[10:13] == [0, 0, 0], c
    assert plan.lib.rv_hook_b3_plan(1024, 1024, 64, 0, 3, 0, (C.c_uint32 * 13)()) == E_ARG  # (quad words without a list)
    assert plan.lib.rv_hook_b3_plan(1024, 1024, 0, 0, 0, 0, (C.c_uint32 * 13)()) == E_ARG


@pytest.mark.parametrize("batch", [0, 1, 7, 8])
def test_tree_plan(plan, batch):
    lane_or_64 = LANE if batch >= 8 else TAIL64
    want = {
        1: (0, 1, LANE), 2: (0, 2, LANE), 4: (0, 4, LANE), 5: (0, 5, lane_or_64), 64: (0, 64, lane_or_64), 65: (0, 65, TAIL512), 512: (0, 512, TAIL512),
        513: (1, 129, TAIL512), 2048: (1, 512, TAIL512), 2049: (2, 129, TAIL512), 8192: (2, 512, TAIL512), 8193: (3, 129, TAIL512),
    }
    for n, w in want.items():
        got = plan(n, n, 64, batch=batch)
        assert tuple(got[2:5]) == w and tuple(got[5:8]) == w, (n, batch)
        assert tuple(plan(n, 1, 16, batch=batch, exact=False)[5:8]) == w, (n, batch)


def test_small_pair(plan):
    for NQ in (8, 64):
        assert plan(64, 64, NQ)[8] == PAIR_Q and plan(1, 64, NQ)[8] == PAIR_Q and plan(64, 1, NQ)[8] == PAIR_Q
        assert plan(65, 1, NQ)[8] == 0 and plan(1, 65, NQ)[8] == 0
        assert plan(0, 0, NQ)[8] == PAIR_Q
        assert plan(64, 64, NQ, n_quads=1)[8] == PAIR_Q and plan(64, 65, NQ, n_quads=1)[8] == 0
    # a recorder: the lane form, and max(chunks) x NQ x batch below 64 x 1024
    assert plan(64, 64, 64, batch=1)[8] == PAIR_LANE and plan(64, 64, 64, batch=2)[8] == PAIR_LANE
    assert plan(63, 1, 64, batch=16)[8] == PAIR_LANE and plan(64, 1, 64, batch=16)[8] == 0 and plan(1, 64, 64, batch=16)[8] == 0
    assert plan(3, 3, 64, batch=256)[8] == PAIR_LANE and plan(3, 4, 64, batch=256)[8] == 0
    assert plan(64, 64, 8, batch=64)[8] == PAIR_LANE and plan(64, 64, 8, batch=128)[8] == 0


def test_big_pair(plan):
    lanes = LANES // 64  # 2 048 chunks of full rows reach the lane threshold
    ok = plan(lanes, lanes)
    assert ok[9] == 1 and ok[10:13] == [3, 256, 256]                   # 2 048 -> 256 nodes each: one shared reduction
    assert plan(lanes - 1, lanes)[9] == 0 and plan(lanes, lanes - 1)[9] == 0   # either stream short: the separate launchers
    assert plan(lanes, lanes, batch=1)[9] == 0 and plan(lanes, lanes, batch=8)[9] == 0  # a recorder present
    assert plan(8192, 8192, NQ=16)[9] == 0 and plan(8192, 8192, NQ=32)[9] == 0   # not full rows
    assert plan(lanes, lanes, n_quads=0)[9] == 0
    # a listed online stream: a quarter of the row or less is hashed a repetition per lane whatever its length, so only its tree decides
    # -- more than 64 nodes must be left for the shared top
    assert plan(lanes, 64, n_quads=16)[9] == 0
    got = plan(lanes, 65, n_quads=16)
    assert got[9] == 1 and got[10:13] == [3, 256, 65]                  # (the online stream sits the reduction out)
    assert plan(lanes, 8 * 64, n_quads=1)[9:13] == [1, 3, 256, 512] and plan(lanes, 1024, n_quads=16)[9:13] == [1, 3, 256, 1024]
    assert plan(lanes, 1025, n_quads=16)[9:13] == [1, 3, 256, 129]
    # a longer list counts its quad words against the lane threshold
    edge = -(-LANES // 17)
    assert plan(lanes, edge - 1, n_quads=17)[9] == 0 and plan(lanes, edge, n_quads=17)[9] == 1
    # launches: chunk launch + shared reductions (three levels each, while a stream has more than 1 024 nodes) + the shared top
    assert plan(8192, 8192)[9:13] == [1, 3, 1024, 1024]
    assert plan(8193, 8192)[9:13] == [1, 4, 129, 1024]               # (the second stream sits the second reduction out)
    assert plan(8193, 2048)[9:13] == [1, 4, 129, 256]
    assert plan(2048, 65537)[9:13] == [1, 5, 256, 129]                 # 65 537 -> 8 193 -> 1 025 -> 129


def test_config4_shape(plan):
    """the 10^7-gate headline circuit: 4 900 online chunks are 613 nodes after ONE shared reduction -- three launches"""
    got = plan(4900, 4900)
    assert got[9:13] == [1, 3, 613, 613]
    assert got[0] == UNI and got[1] == UNI and got[2:5] == [2, 307, TAIL512]  # (the separate launchers would take four launches a stream)
    got = plan(4900, 4900, n_quads=40)
    assert got[0] == RPL4 and got[9:13] == [1, 3, 613, 613]
