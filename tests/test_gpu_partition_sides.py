"""Every even side from 2 to 72 through dxv_partition on the GPU for both kinds at cap_sq 10 (tests/grid_sides.py: the sides, the grids and why
these).  The header's routines are run at the same sides on the CPU by tests/test_partition_rule.py; what exists only in partition.hip -- the wave
per brick with its partial bricks at N % 4 = 2, the mips' wave maxima, the blocks' scans, the wave-wide stats, the sort and the atomics of the
throats -- runs here.  Each grid is written through the frame's grid pointer; labels, table and throats are compared as bytes with the numpy
restatement (form (a))."""
import pytest

import grid_sides as gs
import partition_restated as pr
from raycast_restated import write_grid

pytestmark = pytest.mark.gpu
CAP = 10


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
    """labels, table and throats of both kinds of the selected frame's grid, which holds g, against the restatement"""
    for of in (pr.SOLID, pr.EMPTY):
        want = pr.partition(g, of, CAP)
        got = v.Partition(of, CAP)
        for a, b, what in zip(got, want, ("labels", "table", "throats")):
            assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes(), (N, name, of, what)


@pytest.mark.parametrize("N", gs.SWEEP)
def test_both_kinds_at_every_side(writer, N):
    v = writer
    v.Voxelize(N)
    seen = 0
    for name, g in gs.grids(N):
        seen += 1
        write_grid(v, g)
        check_both_kinds(v, N, name, g)
    assert seen == (5 if N >= 6 else 4)
