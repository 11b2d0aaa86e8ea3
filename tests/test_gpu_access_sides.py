"""Every even side from 2 to 72, and three longer rows, through dxv_access on the GPU with the intrusion map, for both kinds and both
connectivities, seeded from the border and from the single voxel [smallest member index], whose front crosses every tile (tests/grid_sides.py:
the sides, the grids and why these).  The header's routines are run on the CPU by tests/test_access_rule.py, which holds them to the
restatements; what exists only in access.hip -- the wave's load of a tile with its halo, partial tiles where the side is no multiple of 8, the
lanes' columns and their radii, the vote, the write-back, the flags' double buffer, the queue, the batches, the radius field for the paint --
runs here.  Each grid is written through the frame's grid pointer; maps, histograms and the whole tally are compared with the host library.
  2 .. 26         every grid of the sweep at cap 65.
  28 .. 72        "random 0.3" and "ends" at cap 65, every kind, connectivity and seeding: from 66 the tally's strided loop takes a second trip
                  (N^3 > 1024 * 256) and a row of the distance passes has a second word.
  126, 130, 194   "all 0xFF" and "ends" at cap 6, as test_gpu_thickness_sides.py, one item per grid and kind: the histogram's second trip and
                  more than 1024 block sums (chunk 2 of the scan) out of access's own scratch layout, from 102.
The host library takes 0.03 .. 0.10 s per call at side 72 (16 calls in the item: 1.0 s) and 0.6 .. 1.45 s per call at 194 (4 calls in an item:
5.8 s at the most; 0.4 s a call at 130)."""
import numpy as np
import pytest

import access_host as ah
import access_restated as ar
import grid_sides as gs
from raycast_restated import write_grid

pytestmark = pytest.mark.gpu
TALLY = ("seeds_used", "reached", "unreached", "widest", "widest_voxel")
SIDES = list(range(2, 27, 2))


@pytest.fixture(scope="module")
def writer(dxvlib, bunny):
    """the one Voxelizer, on the bunny, whose frame every grid of this file is written into"""
    import dxrvoxelizer_amd
    vb, ib, _ = bunny
    v = dxrvoxelizer_amd.Voxelizer(0)
    v.InitFromArrays(vb, ib)
    yield v
    v.close()


@pytest.mark.parametrize("N", SIDES)
def test_both_kinds_and_both_connectivities_at_every_side(writer, N):
    v = writer
    v.Voxelize(N)
    seen = 0
    for name, g in gs.grids(N):
        seen += 1
        write_grid(v, g)
        for of in (ar.SOLID, ar.EMPTY):
            for connectivity in (6, 26):
                for seeds in ("border", np.flatnonzero(ar.members(g, of).reshape(-1))[:1].astype(np.uint32)):
                    key = (N, name, of, connectivity, type(seeds))
                    want = ah.access(g, of, connectivity, 65, seeds)
                    A, I = v.Access(of, connectivity, 65, seeds)
                    assert A.tobytes() == want["A"].tobytes() and I.tobytes() == want["I"].tobytes(), key
                    assert v.AccessHistogram().tobytes() == want["hist_a"].tobytes() and v.IntrusionHistogram().tobytes() == want["hist_i"].tobytes(), key
                    info = v.AccessInfo()
                    assert {k: info[k] for k in TALLY} == want["tally"], key
    assert seen == (5 if N >= 6 else 4)


def check_connectivities_and_seeds(v, N, name, g, of, cap):
    """A, I, both histograms and the tally of one kind of the selected frame's grid, which holds g, for both connectivities and both seedings"""
    for connectivity in (6, 26):
        for seeds in ("border", np.flatnonzero(ar.members(g, of).reshape(-1))[:1].astype(np.uint32)):
            key = (N, name, of, connectivity, type(seeds))
            want = ah.access(g, of, connectivity, cap, seeds)
            A, I = v.Access(of, connectivity, cap, seeds)
            assert A.tobytes() == want["A"].tobytes() and I.tobytes() == want["I"].tobytes(), key
            assert v.AccessHistogram().tobytes() == want["hist_a"].tobytes() and v.IntrusionHistogram().tobytes() == want["hist_i"].tobytes(), key
            info = v.AccessInfo()
            assert {k: info[k] for k in TALLY} == want["tally"], key


@pytest.mark.parametrize("N", [N for N in gs.SWEEP if N > SIDES[-1]])
def test_two_grids_at_the_sweeps_other_sides(writer, N):
    v = writer
    v.Voxelize(N)
    seen = 0
    for name, g in gs.grids(N, ("random 0.3", "ends")):
        seen += 1
        write_grid(v, g)
        for of in (ar.SOLID, ar.EMPTY):
            check_connectivities_and_seeds(v, N, name, g, of, 65)
    assert seen == 2


@pytest.mark.parametrize("of", [ar.SOLID, ar.EMPTY])
@pytest.mark.parametrize("name", ["all 0xFF", "ends"])
@pytest.mark.parametrize("N", gs.WIDE)
def test_the_longer_rows(writer, N, name, of):
    v = writer
    if v.stats()["grid_dim"] != N:
        v.Voxelize(N)
    g = dict(gs.grids(N, (name,)))[name]
    write_grid(v, g)
    check_connectivities_and_seeds(v, N, name, g, of, 6)
