"""Every operator of a frame's grid in the scratch an earlier, larger grid left behind.  DevBuf::reserve (csrc/dxv_ctx.h) keeps an allocation
whenever it is large enough, and the sides files walk their one Voxelizer upwards, so there every side runs in fresh memory; a caller who
voxelizes at 72 and then at 70 runs in masks whose rows have the same word count with bits 70 and 71 still set, at 38 in one-word rows read
out of memory that held two-word rows, and in control blocks, counters, flags, queues, histograms and product buffers that hold the larger
grid's values.  What exists only in the .hip files and in the launch code -- which of these a launch clears, and that it is enough -- runs
here.  Each test dirties its operator's scratch at side 72 ("all 0xFF", then "random 0.6"), goes down through 70, 66, 38, 12, 6 and 2 with
"random 0.3" and "ends", and comes back up to 72 with "random 0.3"; every result is compared as the operator's sides file compares it, by its
own helpers: array_equal or byte equality, no tolerance.  After each operator that edits the grid the whole grid is read back.  (The thin's
share is in tests/test_gpu_thin_sides.py, after 194; the launch paths after a larger grid are tests/test_gpu_parity.py's.)"""
import functools

import numpy as np
import pytest

import components_restated as cr
import grid_sides as gs
import morph_restated as mr
import test_gpu_components as tgc
import test_gpu_geodesic_sides as tgg
import test_gpu_grid_sides as tgs
import test_gpu_isosurface as tgi
import test_gpu_measure as tgm
import test_gpu_octree as tgo
import test_gpu_partition_sides as tgp
import test_gpu_thickness_sides as tgt
from raycast_restated import write_grid
from test_gpu_distance import check_field

pytestmark = pytest.mark.gpu

TOP = 72
DIRTY = ((TOP, "all 0xFF"), (TOP, "random 0.6"))
DESCENT = tuple((N, name) for N in (70, 66, 38, 12, 6, 2) for name in ("random 0.3", "ends"))
BACK_UP = ((TOP, "random 0.3"),)
PLAN = DIRTY + DESCENT + BACK_UP

assert {N for N, _ in DESCENT} >= {70, 66, 38, 6, 2} and {name for _, name in DESCENT} == {"random 0.3", "ends"}


@pytest.fixture(scope="module")
def dxv(dxvlib):
    import dxrvoxelizer_amd
    return dxrvoxelizer_amd


@pytest.fixture(scope="module")
def writer(dxv, bunny):
    """the one Voxelizer, on the bunny, whose frame every grid of this file is written into: each operator has its own scratch"""
    vb, ib, _ = bunny
    v = dxv.Voxelizer(0)
    v.InitFromArrays(vb, ib)
    yield v
    v.close()


@functools.lru_cache(maxsize=None)
def grid(N, name):
    """the sweep's grid of that name at side N, made once for the tests of this file and left unchanged"""
    (_, g), = gs.grids(N, (name,))
    return g


def walk(v, check, plan=PLAN):
    """dirty, descend, back up: check(N, name, g) with g written into the frame at each step of the plan"""
    assert plan[:2] == DIRTY and plan[-1:] == BACK_UP and all(N < TOP for N, _ in plan[2:-1])
    steps, side = 0, None
    for N, name in plan:
        if N != side:
            v.Voxelize(N)
            side = N
        g = grid(N, name)
        write_grid(v, g)
        check(N, name, g)
        steps += 1
    assert steps == len(plan) == (15 if plan is PLAN else 5)


def labelling_key(N, name):
    return f"reuse {name} {N}"


def forget(N, name):
    """the labellings of side 72 are kept for the tests that come back to them; a smaller side's are not needed again"""
    if N != TOP:
        for k in [k for k in tgc._RESTATED if k[0] == labelling_key(N, name)]:
            del tgc._RESTATED[k]


def test_count_bits_and_fill(writer):
    v = writer

    def check(N, name, g):
        what = f"reuse: N = {N}, {name}"
        tgs.check_count_and_bits(v, g, what)
        tgs.check_fill_both_batches(v, g, what)                         # (reads the whole grid back after each fill)
    walk(v, check)


def test_distance_field_in_both_formats(dxv, writer):
    v = writer

    def check(N, name, g):
        got, _ = check_field(v, dxv, f"reuse: N = {N}, {name}")
        assert np.array_equal(got, g), (N, name)
    walk(v, check)


def test_components_solid_6_and_empty_26(writer):
    v = writer

    def check(N, name, g):
        key = labelling_key(N, name)
        try:
            for of, conn in ((cr.SOLID, 6), (cr.EMPTY, 26)):
                tgc.check(v, key, g, of, conn)
            assert np.array_equal(v.Grid(), g), key                     # labelling edits nothing
        finally:
            forget(N, name)
    walk(v, check)


# four labellings and sixteen selections per grid: the whole plan costs five cases of the sides file at 72, so there is a case per side of
# the descent, each between the same dirtying and the same way back up (whose labellings are made once)
@pytest.mark.parametrize("N", sorted({N for N, _ in DESCENT}, reverse=True))
def test_select_components(writer, N):
    v = writer

    def check(N, name, g):
        try:
            tgc.check_select(v, labelling_key(N, name), g)              # (writes the grid before and reads it back after each selection)
        finally:
            forget(N, name)
    walk(v, check, DIRTY + tuple(step for step in DESCENT if step[0] == N) + BACK_UP)


def test_dilate_and_erode_in_both_forms(writer):
    v = writer

    def check(N, name, g):
        tgs.check_morph_both_forms(v, g, (mr.DILATE, mr.ERODE), (10,), f"reuse: N = {N}, {name}")     # (reads the whole grid back after each morph)
    walk(v, check)


def test_octree_and_expansion(writer):
    v = writer

    def check(N, name, g):
        what = f"reuse: N = {N}, {name}"
        nodes = tgo.check(v, g, what)
        assert len(nodes) >= 1
        assert np.array_equal(v.Grid(), g), what                        # the build edits nothing
        write_grid(v, np.full((N, N, N), tgs.POISON, np.uint8))         # poison: every voxel must be written
        v.OctreeExpand()
        assert np.array_equal(v.Grid(), (g != 0).astype(np.uint8)), what
    walk(v, check)


def test_isosurface_of_the_grid_distance_field(dxv, writer):
    v = writer

    def check(N, name, g):
        v.DistanceField(dxv.DIST_F32)
        n = tgi.all_levels_and_spaces(v, dxv, dxv.ISO_GRID_DISTANCE, tgi.F32(1.0), f"reuse: N = {N}, {name}")
        assert n > 0, (N, name)                                         # every grid of the sweep has solid voxels
    walk(v, check)


def test_measure(writer):
    v = writer
    walk(v, lambda N, name, g: tgm.check(v, g, f"reuse: N = {N}, {name}"))


def test_thickness(writer):
    v = writer
    walk(v, lambda N, name, g: tgt.check_both_kinds(v, N, name, g))


def test_partition(writer):
    v = writer
    walk(v, lambda N, name, g: tgp.check_both_kinds(v, N, name, g))


def test_geodesic(writer):
    v = writer
    walk(v, lambda N, name, g: tgg.check_kinds_metrics_and_seeds(v, N, name, g))
