"""Topology-preserving thinning on the GPU (include/dxv.h: dxv_thin*): after a thin every byte of the device's grid equals the numpy restatement
(tests/thin_restated.py) of the grid as it was before -- array_equal, no tolerance, both kinds -- and CountSolid and thin_info's iterations,
removed voxels and verdict agree with it: for meshes, for arbitrary grids written through the frame's grid pointer, across the word
boundaries of a mask row, for bounded runs and every batch size, against the device's own components, for a large grid against committed
hashes (tests/golden/thin.json, tests/gen_thin_fixtures.py), for three frames in flight; the frame state a thin must touch; and the calls
refuse what they must."""
import json
import os

import numpy as np
import pytest

import distance_restated as dr
import fill_restated as fr
import morph_restated as mr
import thin_restated as tr
import thin_shapes as ts
from conftest import GOLD, load_mesh
from raycast_restated import write_grid
from test_gpu_fill import arbitrary_grids

pytestmark = pytest.mark.gpu

_WANT = {}


def restated(key, g, kind, limit=0):
    """tr.thin(g, kind, limit), made once per (key, kind, limit) for the tests that share a grid"""
    k = (key, kind, limit)
    if k not in _WANT:
        _WANT[k] = tr.thin(g, kind, limit)
    return _WANT[k]


@pytest.fixture(scope="module")
def dxv(dxvlib):
    import dxrvoxelizer_amd
    return dxrvoxelizer_amd


def check_thin(v, before, produce, kind, want, what_for, limit=0):
    """`produce()` puts `before` back into the selected frame, Thin(kind, limit), the grid and thin_info against `want` = tr.thin(before, kind, limit)"""
    produce()
    assert v.Thin(kind, limit) is True
    got = v.Grid()
    grid, iterations, removed, converged = want
    assert got.dtype == np.uint8 and np.array_equal(got, grid), (what_for, kind, limit)
    assert v.CountSolid() == int(np.count_nonzero(grid)), (what_for, kind, limit)
    assert v.thin_info()[1:] == (iterations, removed, int(converged)), (what_for, kind, limit, v.thin_info())
    assert removed == tr.counts(before, grid)


# ---- meshes ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["bunny", "dragon", "turingbowl"])
def test_thin_of_mesh_grids_equals_restatement(dxv, name):
    vb, ib, _ = load_mesh(name)
    v = dxv.Voxelizer(0)
    try:
        v.InitFromArrays(vb, ib)
        for mode in (0, 2):
            v.Voxelize(64, mode)
            before = v.Grid()
            assert before.any()
            for kind in tr.KINDS:
                want = restated((name, mode), before, kind)
                check_thin(v, before, lambda: v.Voxelize(64, mode), kind, want, f"{name} mode {mode}")
                assert 0 < int(want[0].sum()) <= int(np.count_nonzero(before))
    finally:
        v.close()


# ---- arbitrary grids ----------------------------------------------------------------------------------------------------------------
# 32 and 2: every grid of the fill's list; 2: every voxel is border and every voxel its own subfield.  64 and 66: one word per row, and a second
# word of two bits with N % 8 != 0
@pytest.mark.parametrize("N", [32, 2, 64, 66])
def test_thin_of_arbitrary_grids_equals_restatement(dxv, bunny, N):
    vb, ib, _ = bunny
    v = dxv.Voxelizer(0)
    try:
        v.InitFromArrays(vb, ib)
        v.Voxelize(N)
        large = ("all 0xFF", "one voxel", "checkerboard", "maze", "random 0.3")
        seen, other_bytes = set(), False
        for what, g in arbitrary_grids(N):
            if N >= 64 and what not in large:
                continue
            seen.add(what)
            other_bytes |= bool((g > 1).any())
            for kind in tr.KINDS:
                check_thin(v, g, lambda: write_grid(v, g), kind, tr.thin(g, kind), f"N = {N}, {what}")
        assert N < 64 or seen == set(large)
        assert other_bytes                                              # (bytes other than 1 were among them)
    finally:
        v.close()


# ---- the word boundaries of a mask row ----------------------------------------------------------------------------------------------
def test_thin_across_the_word_boundaries_of_a_row(dxv, bunny):
    vb, ib, _ = bunny
    g = ts.rods(130)
    assert g[11, 11, 63] and g[11, 11, 64] and g[21, 21, 127] and g[21, 21, 128] and g[31, 34, 64] and g[62, 62, 64]
    v = dxv.Voxelizer(0)
    try:
        v.InitFromArrays(vb, ib)
        v.Voxelize(130)
        for kind in tr.KINDS:
            want = tr.thin(g, kind)
            check_thin(v, g, lambda: write_grid(v, g), kind, want, "rods")
            first = tr.thin(g, kind, 1)                                # the first iteration alone takes voxels at bits 63 and 0 of two words of a row
            went = (g != 0) & (first[0] == 0)
            assert went[:, :, 63].any() and went[:, :, 64].any() and went[:, :, 127].any() and went[:, :, 128].any()
            check_thin(v, g, lambda: write_grid(v, g), kind, first, "rods", limit=1)
    finally:
        v.close()


# ---- bounded runs ---------------------------------------------------------------------------------------------------------------------
def test_max_iterations_stops_it_and_a_second_call_goes_on(dxv, bunny):
    vb, ib, _ = bunny
    v = dxv.Voxelizer(0)
    try:
        v.InitFromArrays(vb, ib)
        v.Voxelize(64, dxv.MODE_SURFACE)
        v.Fill()
        before = v.Grid()
        for kind in tr.KINDS:
            whole = restated("bunny 64 filled", before, kind)
            assert whole[1] > 4
            for limit in (1, 2, 3):
                want = restated("bunny 64 filled", before, kind, limit)
                assert not want[3] and want[1] == limit
                check_thin(v, before, lambda: write_grid(v, before), kind, want, "bunny 64 filled", limit=limit)
                assert v.thin_info()[3] == 0
                assert v.Thin(kind) is True                             # ... and on from there to the fixed point
                assert np.array_equal(v.Grid(), whole[0]), (kind, limit)
                assert v.thin_info()[1:] == (whole[1] - limit, whole[2] - want[2], 1), (kind, limit)
    finally:
        v.close()


# ---- batches ----------------------------------------------------------------------------------------------------------------------------
def test_every_batch_size_gives_the_same_grid_and_counts(dxv, bunny):
    vb, ib, _ = bunny
    v = dxv.Voxelizer(0)
    try:
        v.InitFromArrays(vb, ib)
        v.Voxelize(64, dxv.MODE_SURFACE)
        v.Fill()
        before = v.Grid()
        for kind in tr.KINDS:
            want = restated("bunny 64 filled", before, kind)
            for rounds in (1, 0, 64):
                v.set_option("thinrounds", rounds)
                check_thin(v, before, lambda: write_grid(v, before), kind, want, f"thinrounds {rounds}")
                check_thin(v, before, lambda: write_grid(v, before), kind, restated("bunny 64 filled", before, kind, 5), f"thinrounds {rounds}", limit=5)
        with pytest.raises(dxv.DxvError, match="thinrounds"):
            v.set_option("thinrounds", 65)
    finally:
        v.close()


def test_what_comes_behind_an_unsettled_thin_settles_it_first(dxv, bunny):
    vb, ib, _ = bunny
    v = dxv.Voxelizer(0)
    try:
        v.InitFromArrays(vb, ib)
        v.set_option("thinrounds", 1)                                  # the thin is still unsettled when the next operator is asked for
        v.Voxelize(64, dxv.MODE_SURFACE)
        v.Fill()
        before = v.Grid()
        want = restated("bunny 64 filled", before, tr.CURVE)
        thinned = want[0]
        # a morph
        write_grid(v, before)
        assert v.Thin(dxv.THIN_CURVE, sync=False) is True
        assert v.Morph(dxv.MORPH_DILATE, 1, sync=False) is True
        v.Sync()
        assert v.thin_info()[1:] == (want[1], want[2], 1) and want[1] > 1
        assert np.array_equal(v.Grid(), mr.morph(thinned, mr.DILATE, 1))
        # components
        write_grid(v, before)
        assert v.Thin(dxv.THIN_CURVE, sync=False) is True
        assert v.Components(dxv.COMP_SOLID, 26, sync=False) is True
        v.Sync()
        assert v.thin_info()[1] == want[1] > 1
        assert np.array_equal(v.ComponentLabels() != 0, thinned != 0) and np.array_equal(v.Grid(), thinned)
        # a distance field
        write_grid(v, before)
        assert v.Thin(dxv.THIN_CURVE, sync=False) is True
        assert v.DistanceField(dxv.DIST_SQ_I32, sync=False) is True
        v.Sync()
        assert v.thin_info()[1] == want[1] > 1
        assert np.array_equal(v.Distance(), dr.distance_sq(thinned)) and np.array_equal(v.Grid(), thinned)
        # a second thin, of the other kind: from the first one's fixed point
        write_grid(v, before)
        assert v.Thin(dxv.THIN_CURVE, sync=False) is True
        assert v.Thin(dxv.THIN_KERNEL, sync=False) is True
        v.Sync()
        assert np.array_equal(v.Grid(), tr.thin(thinned, tr.KERNEL)[0])
        # a thin behind an unsettled fill
        v.set_option("fillrounds", 1)
        v.Voxelize(64, dxv.MODE_SURFACE, sync=False)
        assert v.Fill(sync=False) is True
        assert v.Thin(dxv.THIN_CURVE, sync=False) is True
        v.Sync()
        assert v.fill_info()[1] > 1 and np.array_equal(v.Grid(), thinned)
    finally:
        v.close()


# ---- the device's own components as second oracle ----------------------------------------------------------------------------------------
def enclosed(table):
    """the empty 6-components of the grid padded by an empty layer, less the outside: the ones that do not reach the grid's border.  (Voxels
    outside the grid are empty for a thin, so every empty component that reaches the border is one with the outside -- the filled bunny stands on
    the grid's floor and cuts pockets off there that the labelling of the grid alone counts as components of their own, and a thin opens them.)"""
    return int(np.count_nonzero((table["flags"] & 1) == 0))


def test_pieces_and_cavities_counted_on_the_device_do_not_change(dxv, bunny):
    vb, ib, _ = bunny
    v = dxv.Voxelizer(0)
    try:
        v.InitFromArrays(vb, ib)
        left = {}
        for kind in tr.KINDS:
            v.Voxelize(128, dxv.MODE_SURFACE)
            v.Fill()
            solid_before = v.CountSolid()
            pieces, cavities = len(v.Components(dxv.COMP_SOLID, 26)[1]), enclosed(v.Components(dxv.COMP_EMPTY, 6)[1])
            v.Thin(kind)
            assert len(v.Components(dxv.COMP_SOLID, 26)[1]) == pieces >= 1, kind
            assert enclosed(v.Components(dxv.COMP_EMPTY, 6)[1]) == cavities, kind
            left[kind] = v.CountSolid()
            ms, iterations, removed, converged = v.thin_info()
            assert ms > 0.0 and iterations > 1 and removed == solid_before - left[kind] and converged == 1
            once = v.Grid()
            v.Thin(kind)                                                # idempotent
            assert np.array_equal(v.Grid(), once) and v.thin_info()[1:] == (1, 0, 1)
        assert 0 < left[tr.KERNEL] <= left[tr.CURVE]
    finally:
        v.close()


# ---- a large grid against committed hashes ---------------------------------------------------------------------------------------------
def test_thin_of_a_large_grid_equals_committed_hashes(dxv, bunny):
    with open(os.path.join(GOLD, "thin.json")) as fh:
        want = json.load(fh)["bunny/256"]
    vb, ib, _ = bunny
    v = dxv.Voxelizer(0)
    try:
        v.InitFromArrays(vb, ib)
        for kind, tag in zip(tr.KINDS, ("curve", "kernel")):
            v.Voxelize(want["side"], dxv.MODE_SURFACE)
            v.Fill()
            assert v.CountSolid() == want["grid_count"] and tr.packed_sha(v.Grid()) == want["grid_packed_sha256"], "the grid is not the one the fixture was made from"
            v.Thin(kind)
            assert 0 < want[tag]["count"] < want["grid_count"]
            assert v.CountSolid() == want[tag]["count"], tag
            assert tr.packed_sha(v.Grid()) == want[tag]["packed_sha256"], f"{tag}: the count agrees but the grid's hash differs"
            assert v.thin_info()[1:] == (want[tag]["iterations"], want[tag]["removed"], 1), tag
    finally:
        v.close()


# ---- frame state ---------------------------------------------------------------------------------------------------------------------
def test_three_frames_in_flight_each_get_their_own_thin(dxv, bunny):
    vb, ib, _ = bunny
    v = dxv.Voxelizer(0)
    try:
        v.InitFromArrays(vb, ib)
        plan = [(0, 64, dxv.MODE_REFERENCE, dxv.THIN_CURVE, 0), (1, 96, dxv.MODE_SURFACE, dxv.THIN_KERNEL, 0), (2, 48, dxv.MODE_PARITY, dxv.THIN_KERNEL, 2)]
        before = {}
        for frame, N, mode, kind, limit in plan:
            v.Voxelize(N, mode, frameIndex=frame)
            before[frame] = v.Grid()
        for frame, N, mode, kind, limit in plan:                        # no synchronisation between any of these
            v.Voxelize(N, mode, sync=False, frameIndex=frame)
            assert v.Thin(kind, limit, sync=False) is True
        v.SyncAll()
        for frame, N, mode, kind, limit in plan:
            v.SetFrame(frame)
            v.Sync()
            want = tr.thin(before[frame], kind, limit)
            info = v.thin_info()
            assert info[0] > 0.0 and info[1:] == (want[1], want[2], int(want[3])), frame
            got = v.Grid()
            assert got.shape == (N, N, N) and np.array_equal(got, want[0]), frame
    finally:
        v.close()


def test_a_field_and_a_tree_made_before_a_thin_are_stale_after_it(dxv, bunny):
    vb, ib, _ = bunny
    v = dxv.Voxelizer(0)
    try:
        v.InitFromArrays(vb, ib)
        v.Voxelize(64)
        assert v.thin_info() == (0.0, 0, 0, 0)                          # before the first thin
        v.DistanceField(dxv.DIST_SQ_I32)
        v.Octree()
        assert v.distance_device_ptr() and v.OctreeInfo()
        v.Thin(dxv.THIN_CURVE)
        with pytest.raises(dxv.DxvError, match="stale"):
            v.distance_device_ptr()
        with pytest.raises(dxv.DxvError, match="stale"):
            v.OctreeInfo()
        assert np.array_equal(v.DistanceField(dxv.DIST_SQ_I32), dr.distance_sq(v.Grid()))
    finally:
        v.close()


def test_trim_then_thin_is_the_same(dxv, bunny):
    vb, ib, _ = bunny
    v = dxv.Voxelizer(0)
    try:
        v.InitFromArrays(vb, ib)
        v.Voxelize(64)
        before = v.Grid()
        v.Thin(dxv.THIN_CURVE)
        first = v.Grid()
        v.trim()
        assert np.array_equal(v.Grid(), first)                         # the grid stayed
        v.Voxelize(64)
        v.Thin(dxv.THIN_CURVE)
        assert np.array_equal(v.Grid(), first) and np.array_equal(first, restated(("bunny", 0), before, tr.CURVE)[0])
    finally:
        v.close()


# ---- refusals ------------------------------------------------------------------------------------------------------------------------
def test_thin_refuses_with_a_message_and_launches_nothing(dxv, bunny):
    vb, ib, _ = bunny
    v = dxv.Voxelizer(0)
    lib, ctx = v._lib, v._ctx
    try:
        v.InitFromArrays(vb, ib)
        with pytest.raises(dxv.DxvError, match="no grid yet"):         # before any launch
            v.Thin(dxv.THIN_CURVE)
        v.Voxelize(64, z0=16, nz=32)
        slab = v.Grid()
        with pytest.raises(dxv.DxvError, match="not a slab or a share"):
            v.Thin(dxv.THIN_CURVE)
        assert lib.dxv_thin_async(ctx, 0, 0) == 1 and "not a slab or a share" in lib.dxv_last_error(ctx).decode()
        assert np.array_equal(v.Grid(), slab)
        v.VoxelizeInterleaved(64, 1, 2, 8)
        share = v.Grid()
        with pytest.raises(dxv.DxvError, match="not a slab or a share"):
            v.Thin(dxv.THIN_KERNEL)
        assert np.array_equal(v.Grid(), share)
        v.Voxelize(64)
        whole = v.Grid()
        for bad in (2, -1):
            assert lib.dxv_thin_async(ctx, bad, 0) == 1 and "unknown kind" in lib.dxv_last_error(ctx).decode()
            assert lib.dxv_thin(ctx, bad, 0) == 1
        with pytest.raises(dxv.DxvError, match=r"unknown kind 2 \(DXV_THIN_CURVE = 0, DXV_THIN_KERNEL = 1\)"):
            v.Thin(2)
        assert np.array_equal(v.Grid(), whole)                         # none of the refused calls touched the grid
        assert v.thin_info() == (0.0, 0, 0, 0)
        assert lib.dxv_thin_info(ctx, None, None, None, None) == 0
        v.Thin(dxv.THIN_KERNEL)
        assert np.array_equal(v.Grid(), restated(("bunny", 0), whole, tr.KERNEL)[0])
    finally:
        v.close()
