"""Every even side from 2 to 72, and three longer rows, through dxv_thickness on the GPU for both kinds at cap_sq 6 (tests/grid_sides.py: the
sides, the grids and why these).  The header's routines are run at the same sides on the CPU by tests/test_thickness_rule.py; what exists only in
thickness.hip -- the four voxels per thread, the blocks' scan, the two binary searches, the lanes of a slice, the atomic max, the histogram in
LDS -- runs here.  Each grid is written through the frame's grid pointer; map and histogram are compared as bytes.  To side 72 the expectation
is the numpy restatement (form (a)); at the longer rows, with "all 0xFF" and "ends", it is the host library, which the rule test holds to the
restatement (the numpy distance alone takes most of a minute at 194)."""
import pytest

import grid_sides as gs
import thickness_host as th
import thickness_restated as tr
from raycast_restated import write_grid

pytestmark = pytest.mark.gpu
CAP = 6


@pytest.fixture(scope="module")
def writer(dxvlib, bunny):
    """the one Voxelizer, on the bunny, whose frame every grid of this file is written into"""
    import dxrvoxelizer_amd
    vb, ib, _ = bunny
    v = dxrvoxelizer_amd.Voxelizer(0)
    v.InitFromArrays(vb, ib)
    yield v
    v.close()


def expectation(g, of):
    if g.shape[0] in gs.WIDE:
        W, hist, _ = th.thickness(g, of, CAP)
        return W, hist
    W = tr.thickness(g, of, CAP)
    return W, tr.histogram(W, CAP)


def check_both_kinds(v, N, name, g):
    """map and histogram of both kinds of the selected frame's grid, which holds g, against the expectation"""
    for of in (tr.SOLID, tr.EMPTY):
        want, hist = expectation(g, of)
        got = v.Thickness(of, CAP)
        assert got.dtype == want.dtype and got.shape == want.shape and got.tobytes() == want.tobytes(), (N, name, of)
        assert v.ThicknessHistogram().tobytes() == hist.tobytes(), (N, name, of)


@pytest.mark.parametrize("N", gs.SWEEP + gs.WIDE)
def test_both_kinds_at_every_side(writer, N):
    v = writer
    v.Voxelize(N)
    seen = 0
    for name, g in gs.grids(N, ("all 0xFF", "ends") if N in gs.WIDE else None):
        seen += 1
        write_grid(v, g)
        check_both_kinds(v, N, name, g)
    assert seen == (2 if N in gs.WIDE else 5 if N >= 6 else 4)
