"""Every side of the side sweep through dxv_skeleton on the GPU (tests/grid_sides.py: the sides and why these): the sweep's "random 0.3", "ends"
and "all 0xFF" and a sparse random grid at density 0.05, each side after a larger grid in the same frame, so that scratch, labels and tables of
an earlier size are in use again.  The header's routines are run at sides 2 .. 26 on the CPU by tests/test_skeleton_rule.py, which holds them
to the restatements; what exists only in skeleton.hip -- the lanes' nine loads and the carry words at a row's ends, the wave's counts, the two
masks' merges over one parent array, the two kinds' ranks, the atomics of the stats, the tables -- runs here.  Each grid is written through the
frame's grid pointer; labels, tables and the info's counts are compared with the host library, the smaller sides with the set restatement too."""
import numpy as np
import pytest

import grid_sides as gs
import skeleton_host as sh
import skeleton_restated as sr
from raycast_restated import write_grid

pytestmark = pytest.mark.gpu
NAMES = ("random 0.3", "ends", "all 0xFF")


@pytest.fixture(scope="module")
def writer(dxvlib, bunny):
    """the one Voxelizer, on the bunny, whose frame every grid of this file is written into"""
    import dxrvoxelizer_amd
    vb, ib, _ = bunny
    v = dxrvoxelizer_amd.Voxelizer(0)
    v.InitFromArrays(vb, ib)
    yield v
    v.close()


@pytest.mark.parametrize("N", gs.SWEEP + gs.WIDE)
def test_the_skeleton_at_every_side_after_a_larger_grid(writer, N):
    v = writer
    larger = N + 6
    v.Voxelize(larger)
    write_grid(v, sr.random_grid(larger, 0.1, larger))
    v.Skeleton()
    v.Voxelize(N)
    grids = list(gs.grids(N, NAMES)) + [("random 0.05", sr.random_grid(N, 0.05, N))]
    assert len(grids) == 4
    for name, g in grids:
        write_grid(v, g)
        labels, nodes, branches = v.Skeleton()
        want = sh.skeleton(g)
        key = (N, name)
        assert labels.tobytes() == want[0].tobytes() and nodes.tobytes() == want[1].tobytes() and branches.tobytes() == want[2].tobytes(), key
        info = v.SkeletonInfo()
        assert (info["nodes"], info["branches"], info["end_voxels"], info["curve_voxels"], info["junction_voxels"]) == (len(nodes), len(branches)) + want[3], key
        if N <= 40:
            r = sr.by_sets(g)
            assert labels.tobytes() == r[0].tobytes() and nodes.tobytes() == r[1].tobytes() and branches.tobytes() == r[2].tobytes(), key
