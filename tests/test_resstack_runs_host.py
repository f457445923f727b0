"""CPU only: the run planner of the carried-halo form of the fused 64-channel pair (csrc/resstack.hip, CARRY;
``asw_resstack_runs``).  An item's rows are cut into runs, each a head tile followed by steady tiles; a workgroup walks
one run.  Every bound is equality."""
import ctypes

import pytest

from acousticswarms_speech_amd.native import lib

MAXR = 4096


def _runs(T, B, runs_per_item=0, n_cu=256, taps=7, dils=(1, 7)):
    d = (ctypes.c_int32 * 2)(*dils)
    head, steady = ctypes.c_int32(), ctypes.c_int32()
    start, tiles = (ctypes.c_int32 * MAXR)(), (ctypes.c_int32 * MAXR)()
    n = lib().asw_resstack_runs(T, B, taps, d, runs_per_item, n_cu, ctypes.byref(head), ctypes.byref(steady), start, tiles, MAXR)
    assert n <= MAXR
    return n, head.value, steady.value, list(start[:max(n, 0)]), list(tiles[:max(n, 0)])


def _check_cover(T, n, head, steady, start, tiles):
    """the tiles of all runs cover [0, T) exactly once, every run starts with a head tile, lengths differ by <= 1"""
    assert n >= 1 and len(start) == n
    assert max(tiles) - min(tiles) <= 1 and min(tiles) >= 1
    pos = 0
    for r in range(n):
        assert start[r] == pos                       # a run starts where the one before it ends: no gap, no overlap
        for j in range(tiles[r]):
            assert pos < T                           # no empty tile
            pos += head if j == 0 else steady        # the first tile of every run is a head tile
        if r < n - 1:
            assert pos <= T                          # only the item's last tile may be ragged
    assert pos >= T and pos - T < steady             # ... and it reaches the end


@pytest.mark.parametrize("B", [1, 3, 16, 256, 1000])
def test_runs_cover_every_row_once(B):
    for T in list(range(215, 1200, 7)) + [470, 471, 726, 982, 1000, 3010, 24000, 48000, 48128, 100001]:
        for want in (0, 1, 2, 5, 64):
            n, head, steady, start, tiles = _runs(T, B, want)
            assert (head, steady) == (214, 256)
            _check_cover(T, n, head, steady, start, tiles)
            if want > 0:
                assert n == min(want, -(-T // head))  # as asked, while there are tiles to start them with


def test_runs_fill_the_chip_and_keep_the_head_share_small():
    # the benchmark's shape: 4 runs of 47 tiles; the 4 head tiles recompute 4 x 42 of 48 000 rows
    n, head, steady, start, tiles = _runs(48000, 256)
    assert n == 4 and sorted(tiles) == [47, 47, 47, 48]
    # a single item still spreads over the chip, in runs of at least a head and a steady tile
    n, _, _, _, tiles = _runs(3010, 1)
    assert n == 6 and min(tiles) >= 2
    n, _, _, _, tiles = _runs(48000, 1)
    assert n == 102 and min(tiles) >= 2
    # a large batch: one run per item
    assert _runs(48000, 4096)[0] == 1


def test_forms_that_do_not_carry():
    assert _runs(214, 3)[0] == 0                      # a single tile
    assert _runs(5, 3)[0] == 0
    assert _runs(3010, 3, runs_per_item=-1)[0] == 0   # switched off by the caller
    assert _runs(3010, 3, dils=(1, 9))[0] == 0        # 54 carried rows: more than the registers that hold them
    # the other fused pairs of the models: (1, 2) and (2, 4) with 5 taps
    for dils, head in (((1, 2), 248), ((2, 4), 240)):
        n, h, steady, start, tiles = _runs(1500, 3, taps=5, dils=dils)
        assert h == head
        _check_cover(1500, n, h, steady, start, tiles)
