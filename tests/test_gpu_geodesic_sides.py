"""Every even side from 2 to 72, and three longer rows, through dxv_geodesic on the GPU for both kinds and both metrics, seeded from the border and
from the single voxel [smallest member index], whose front crosses every tile (tests/grid_sides.py: the sides, the grids and why these).  The
header's routines are run at the same sides on the CPU by tests/test_geodesic_rule.py; what exists only in geodesic.hip -- the wave's load of a
tile with its halo, partial tiles where the side is no multiple of 8, the lanes' columns, the vote, the write-back, the flags' double buffer,
the queue, the batches -- runs here.  Each grid is written through the frame's grid pointer; map bytes and the whole tally are compared with
the numpy relaxation (form (a)) to side 40 and with the host library above, which the rule test holds to Dijkstra at every side."""
import pytest

import geodesic_host as gh
import geodesic_restated as gr
import grid_sides as gs
from raycast_restated import write_grid

pytestmark = pytest.mark.gpu
TALLY = ("seeds_used", "reached", "unreached", "farthest", "farthest_voxel")


@pytest.fixture(scope="module")
def writer(dxvlib, bunny):
    """the one Voxelizer, on the bunny, whose frame every grid of this file is written into"""
    import dxrvoxelizer_amd
    vb, ib, _ = bunny
    v = dxrvoxelizer_amd.Voxelizer(0)
    v.InitFromArrays(vb, ib)
    yield v
    v.close()


def expectation(g, of, metric, seeds):
    if g.shape[0] > 40:
        want, tally, _ = gh.geodesic(g, of, metric, seeds)
        return want, tally
    want = gr.geodesic(g, of, metric, seeds)
    return want, gr.tally(want)


def check_kinds_metrics_and_seeds(v, N, name, g):
    """map and tally of both kinds, both metrics and both seedings of the selected frame's grid, which holds g, against the expectation"""
    for of in (gr.SOLID, gr.EMPTY):
        for metric in (gr.FACES, gr.CHAMFER):
            for seeds in (gr.smallest_member(g, of), "border"):
                want, tally = expectation(g, of, metric, seeds)
                got = v.Geodesic(of, metric, seeds)
                assert got.dtype == want.dtype and got.shape == want.shape and got.tobytes() == want.tobytes(), (N, name, of, metric, type(seeds))
                info = v.GeodesicInfo()
                assert {k: info[k] for k in TALLY} == tally, (N, name, of, metric, type(seeds))


@pytest.mark.parametrize("N", gs.SWEEP + gs.WIDE)
def test_both_kinds_and_both_metrics_at_every_side(writer, N):
    v = writer
    v.Voxelize(N)
    seen = 0
    for name, g in gs.grids(N, ("all 0xFF", "ends") if N in gs.WIDE else None):
        seen += 1
        write_grid(v, g)
        check_kinds_metrics_and_seeds(v, N, name, g)
    assert seen == (2 if N in gs.WIDE else 5 if N >= 6 else 4)
