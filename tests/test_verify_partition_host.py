"""rv_verify_partition (host only, no GPU): how rv_verify_sharded deals the verifier's 32 groups of eight slots over the ranks.
Every group exactly once, 32 / world per rank, the 5 online groups round-robin and listed first."""
import ctypes as C

import numpy as np
import pytest

from reverie_amd import _lib
from reverie_amd.dist import verify_partition

WORLDS = [1, 2, 4, 8, 16, 32]
ONLINE_GROUPS = 5


@pytest.mark.parametrize("world", WORLDS)
def test_partition_covers_every_group_once(world):
    parts = [verify_partition(world, r) for r in range(world)]
    assert sorted(g for p in parts for g in p) == list(range(32))
    for r, p in enumerate(parts):
        assert len(p) == 32 // world
        on = [g for g in p if g < ONLINE_GROUPS]
        assert p[:len(on)] == on, "online groups come first"
        assert on == list(range(r, ONLINE_GROUPS, world)), "online groups are dealt round-robin"
        assert len(on) <= -(-ONLINE_GROUPS // world)


def test_partition_examples():
    assert verify_partition(1, 0) == list(range(32))
    assert verify_partition(8, 0) == [0, 5, 6, 7]
    assert verify_partition(8, 4) == [4, 17, 18, 19]
    assert verify_partition(8, 5) == [20, 21, 22, 23]
    assert verify_partition(8, 7) == [28, 29, 30, 31]
    assert [verify_partition(32, r) for r in range(32)] == [[r] for r in range(32)]


def test_partition_argument_errors():
    L = _lib.lib()
    g = np.zeros(32, np.uint8)
    n = C.c_uint32()
    p = g.ctypes.data_as(C.c_void_p)
    for world, rank in [(0, 0), (3, 0), (5, 1), (6, 0), (64, 0), (-1, 0), (2, 2), (2, -1), (8, 8), (1, 1)]:
        assert L.rv_verify_partition(C.c_int(world), C.c_int(rank), p, C.byref(n)) == 9, (world, rank)  # RV_E_ARG
    assert L.rv_verify_partition(C.c_int(2), C.c_int(0), None, C.byref(n)) == 9
    assert L.rv_verify_partition(C.c_int(2), C.c_int(0), p, None) == 9
    with pytest.raises(_lib.ReverieError):
        verify_partition(3, 0)
