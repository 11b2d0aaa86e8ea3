"""Every even side from 2 to 72, and three longer rows, through dxv_sight on the GPU for both kinds and all 26 directions (tests/grid_sides.py:
the sides, the grids and why these).  The header's routines are run on the CPU by tests/test_sight_rule.py, which holds them to the
restatements; what exists only in sight.hip -- the pack from 8-byte loads or guarded bytes, the lanes' families and row groups, the shuffles,
the blocks of loads in front of the chain and their tails, the wave's trip over eight mask words, the tally's reduction -- runs here.  Each grid
is written through the frame's grid pointer; map and tally are compared with the host library and with restatement (b).
  2 .. 72         "random 0.3", "ends" (bytes other than 0 / 1), "hollow box" and "all 0xFF": one word to a row up to 64, two from 66; every
                  N % 8, so every tail of a block of eight steps
  126, 130, 194   "random 0.6", "all 0xFF" and "ends": row groups of 2 and 4 lanes, the third word in a group of four, a last word of 62 bits
                  and of 2
The host library takes 0.2 s per call at side 72 and 2 s at 194, the restatement 0.5 s at 194."""
import numpy as np
import pytest

import grid_sides as gs
import sight_host as sh
import sight_restated as sr
from raycast_restated import write_grid

pytestmark = pytest.mark.gpu
NAMES = ("random 0.3", "ends", "hollow box", "all 0xFF")


@pytest.fixture(scope="module")
def writer(dxvlib, bunny):
    """the one Voxelizer, on the bunny, whose frame every grid of this file is written into"""
    import dxrvoxelizer_amd
    vb, ib, _ = bunny
    v = dxrvoxelizer_amd.Voxelizer(0)
    v.InitFromArrays(vb, ib)
    yield v
    v.close()


def check_both_kinds(v, N, name, g):
    for of in (sr.SOLID, sr.EMPTY):
        want_map, want_tally = sh.sight(g, of, sr.ALL)
        restated = sr.sight(g, of, sr.ALL)                             # (b): the host library is not the only reference at any side
        want = sr.tally(g, of, restated, sr.ALL)
        field = v.Sight(of, sr.ALL)
        assert field.tobytes() == want_map.tobytes() == restated.tobytes(), (N, name, of, int(np.count_nonzero(field != want_map)))
        tally = v.SightTally()
        assert sr.same_tally(tally, want_tally) and sr.same_tally(tally, want), (N, name, of, tally, want_tally)
        if name == "random 0.3" and N >= 16:                            # (the conditions, from the restatement: no degenerate input)
            assert np.count_nonzero(want["count"]) >= 10 and len({int(want["seen"][b]) for b in sr.BITS}) >= 2, (N, of)


@pytest.mark.parametrize("N", gs.SWEEP)
def test_both_kinds_at_every_side(writer, N):
    v = writer
    v.Voxelize(N)
    seen = 0
    for name, g in gs.grids(N, NAMES):
        seen += 1
        write_grid(v, g)
        check_both_kinds(v, N, name, g)
    assert seen == (4 if N >= 6 else 3)


@pytest.mark.parametrize("name", gs.WIDE_GRIDS)
@pytest.mark.parametrize("N", gs.WIDE)
def test_the_longer_rows(writer, N, name):
    v = writer
    if v.stats()["grid_dim"] != N:
        v.Voxelize(N)
    g = dict(gs.grids(N, (name,)))[name]
    write_grid(v, g)
    check_both_kinds(v, N, name, g)
