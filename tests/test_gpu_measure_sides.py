"""Every even side from 2 to 72, and three longer rows, through dxv_measure on the GPU for both kinds and both connectivities (tests/grid_sides.py:
the sides, the grids and why these).  The header's routines are run at the same sides on the CPU by tests/test_measure_rule.py; what exists
only in measure.hip -- the lane per mask word, the wave's loop over runs and its one-label reduction, the atomics, the total -- runs here.
Each grid is written through the frame's grid pointer and the whole table is compared as bytes with the numpy restatement.  The grids of a
side are the ones tests/test_measure_rule.py takes there: all of the sweep's to side 72, "all 0xFF" and "ends" at the longer rows."""
import pytest

import grid_sides as gs
from raycast_restated import write_grid
from test_gpu_measure import check

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def writer(dxvlib, bunny):
    """the one Voxelizer, on the bunny, whose frame every grid of this file is written into"""
    import dxrvoxelizer_amd
    vb, ib, _ = bunny
    v = dxrvoxelizer_amd.Voxelizer(0)
    v.InitFromArrays(vb, ib)
    yield v
    v.close()


def names_at(N):
    return ("all 0xFF", "ends") if N in gs.WIDE else None


@pytest.mark.parametrize("N", gs.SWEEP + gs.WIDE)
def test_both_kinds_and_connectivities_at_every_side(writer, N):
    v = writer
    v.Voxelize(N)
    seen = 0
    for name, g in gs.grids(N, names_at(N)):
        seen += 1
        write_grid(v, g)
        check(v, g, f"N = {N}, {name}")
    assert seen == (2 if N in gs.WIDE else 5 if N >= 6 else 4)
