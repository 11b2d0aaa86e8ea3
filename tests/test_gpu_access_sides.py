"""Every even side from 2 to 26 through dxv_access on the GPU with the intrusion map, for both kinds and both connectivities, seeded from the
border and from the single voxel [smallest member index], whose front crosses every tile (tests/grid_sides.py: the grids and why these).  The
header's routines are run at the same sides on the CPU by tests/test_access_rule.py, which holds them to the restatements; what exists only in
access.hip -- the wave's load of a tile with its halo, partial tiles where the side is no multiple of 8, the lanes' columns and their radii, the
vote, the write-back, the flags' double buffer, the queue, the batches, the radius field for the paint -- runs here.  Each grid is written
through the frame's grid pointer; maps, histograms and the whole tally are compared with the host library."""
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
