"""Every even side from 2 to 72, and three longer rows, through both kinds of dxv_thin on the GPU (tests/grid_sides.py: the sides, the grids and
why these).  The header's routines are run at the same sides on the CPU by tests/test_thin_rule.py; what exists only in thin.hip -- the
kernels' own indexing of a quarter of the rows, the neighbour words at a row's ends, the launch geometry, the 8-byte and the guarded byte
path of pack and write-back -- runs here.  Each grid is written through the frame's grid pointer and the whole grid is compared with the numpy
restatement by array_equal, with iterations and removed voxels beside it, to the fixed point and stopped after two iterations.  The random grids
stop at side 32 and the longer rows take "all 0xFF" and "ends", for the restatement's sake (tests/test_thin_rule.py has its times)."""
import numpy as np
import pytest

import grid_sides as gs
import thin_restated as tr
from raycast_restated import write_grid
from test_gpu_thin import check_thin

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
    if N in gs.WIDE:
        return ("all 0xFF", "ends")
    return ("all 0xFF", "ends", "hollow box") + (("random 0.6", "random 0.3") if N <= 32 else ())


@pytest.mark.parametrize("N", gs.SWEEP + gs.WIDE)
def test_both_kinds_at_every_side(writer, N):
    v = writer
    v.Voxelize(N)
    seen = 0
    for name, g in gs.grids(N, names_at(N)):
        seen += 1
        for kind in tr.KINDS:
            check_thin(v, g, lambda: write_grid(v, g), kind, tr.thin(g, kind), f"N = {N}, {name}")
            if N not in gs.WIDE:
                check_thin(v, g, lambda: write_grid(v, g), kind, tr.thin(g, kind, 2), f"N = {N}, {name}", limit=2)
    assert seen == len(names_at(N)) - (1 if N < 6 else 0)               # (no hollow box below side 6)
    full = tr.thin(np.full((N, N, N), 0xFF, np.uint8), tr.KERNEL)
    assert int(full[0].sum()) == 1 and full[2] == N ** 3 - 1            # an all-solid grid thins from its border, down to one voxel
