"""Morphology by the Euclidean ball on the GPU (include/dxv.h: dxv_morph*): after a morph every byte of the device's grid equals the numpy
restatement (tests/morph_restated.py) of the grid as it was before -- array_equal, no tolerance, all four operations -- and CountSolid and
morph_info's counts agree with it: for meshes, for arbitrary grids written through the frame's grid pointer, at the far end of the radius
range, against the device's own distance field, for a large grid against committed hashes (tests/golden/morph.json,
tests/gen_morph_fixtures.py), for the sealing recipe, for three frames in flight; the frame state a morph must touch; and the calls refuse
what they must."""
import json
import os

import numpy as np
import pytest

import distance_restated as dr
import fill_restated as fr
import morph_restated as mr
from conftest import GOLD, load_mesh
from raycast_restated import write_grid
from test_gpu_fill import arbitrary_grids

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dxv(dxvlib):
    import dxrvoxelizer_amd
    return dxrvoxelizer_amd


def check_morph(v, before, produce, op, r2, want, what_for):
    """`produce()` puts `before` back into the selected frame, Morph(op, r2), the grid and the counts against `want`"""
    produce()
    assert v.Morph(op, r2) is True
    got = v.Grid()
    assert got.dtype == np.uint8 and np.array_equal(got, want), (what_for, op, r2)
    assert v.CountSolid() == int(np.count_nonzero(want)), (what_for, op, r2)
    assert v.morph_info()[1:] == mr.counts(before, want), (what_for, op, r2)


# ---- meshes ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["bunny", "dragon", "turingbowl"])
def test_morph_of_mesh_grids_equals_restatement(dxv, name):
    vb, ib, _ = load_mesh(name)
    v = dxv.Voxelizer(0)
    try:
        v.InitFromArrays(vb, ib)
        for mode in (0, 2):
            v.Voxelize(64, mode)
            before = v.Grid()
            assert before.any()
            for r2 in (1, 3, 4, 9):
                for op in mr.OPS:
                    check_morph(v, before, lambda: v.Voxelize(64, mode), op, r2, mr.morph(before, op, r2), f"{name} mode {mode}")
    finally:
        v.close()


# ---- arbitrary grids ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [64, 96, 66, 2])      # one word per row; one and a half; a second word of two bits (N % 8 != 0); all border
def test_morph_of_arbitrary_grids_equals_restatement(dxv, bunny, N):
    vb, ib, _ = bunny
    v = dxv.Voxelizer(0)
    try:
        v.InitFromArrays(vb, ib)
        v.Voxelize(N)
        for what, g in arbitrary_grids(N):
            for r2 in (1, 2, 4, 10, 27):
                for op in mr.OPS:
                    check_morph(v, g, lambda: write_grid(v, g), op, r2, mr.morph(g, op, r2), f"N = {N}, {what}")
    finally:
        v.close()


# ---- the far end of the range ----------------------------------------------------------------------------------------------------------
FAR_N = 130


def far_grid(gap):
    """a voxel and, `gap` voxels from it along each axis, three more; along x the pair lies across a word boundary"""
    g = np.zeros((FAR_N, FAR_N, FAR_N), np.uint8)
    g[3, 5, 60] = 1
    g[3 + gap, 5, 60] = g[3, 5 + gap, 60] = g[3, 5, 60 + gap] = 0x80
    return g


@pytest.fixture(scope="module")
def far_fields():
    """gap -> (the grid, its restated squared distance field): made once, thresholded by the tests"""
    return {gap: (far_grid(gap), dr.distance_sq(far_grid(gap))) for gap in (64, 65)}


@pytest.mark.parametrize("form", [1, 2])                                # the bit planes, which the radius alone would not pick here, and the field form
@pytest.mark.parametrize("gap", [64, 65])
def test_morph_at_the_far_end_of_the_range(dxv, bunny, far_fields, gap, form):
    vb, ib, _ = bunny
    g, d = far_fields[gap]
    solid = g != 0
    v = dxv.Voxelizer(0)
    try:
        v.InitFromArrays(vb, ib)
        v.Voxelize(FAR_N)
        v.set_option("morphform", form)
        for r2 in (4095, 4096):
            dilated = (solid | (d <= r2)).astype(np.uint8)
            eroded = (solid & (-d.astype(np.int64) > r2)).astype(np.uint8)
            check_morph(v, g, lambda: write_grid(v, g), mr.DILATE, r2, dilated, f"gap {gap}")
            check_morph(v, g, lambda: write_grid(v, g), mr.ERODE, r2, eroded, f"gap {gap}")
            assert not eroded.any()
    finally:
        v.close()


def test_a_voxel_at_distance_64_is_set_at_4096_and_not_at_4095(dxv, bunny):
    vb, ib, _ = bunny
    one = np.zeros((FAR_N, FAR_N, FAR_N), np.uint8)
    one[1, 2, 3] = 1
    v = dxv.Voxelizer(0)
    try:
        v.InitFromArrays(vb, ib)
        v.Voxelize(FAR_N)
        for form in (0, 1, 2):
            v.set_option("morphform", form)
            for r2, reached in ((4095, 0), (4096, 1)):
                write_grid(v, one)
                v.Morph(mr.DILATE, r2)
                out = v.Grid()
                assert out[65, 2, 3] == reached and out[1, 66, 3] == reached and out[1, 2, 67] == reached, (form, r2)
                assert out[64, 2, 3] == 1 and out[1, 65, 3] == 1 and out[1, 2, 66] == 1 and out[1, 2, 68] == 0 and out[66, 2, 3] == 0, (form, r2)
    finally:
        v.close()


def far_halves_grids():
    """66^3, where a ball of radius 64 still has room: two voxels far apart (CLOSE joins what lies between them), and an all-solid grid with
    one empty corner voxel (ERODE leaves what is farther than the radius from it, OPEN grows that back)"""
    pair = np.zeros((66, 66, 66), np.uint8)
    pair[1, 2, 3] = 1
    pair[64, 60, 62] = 0x80
    corner = np.full((66, 66, 66), 0xFF, np.uint8)
    corner[0, 0, 0] = 0
    return {"pair": pair, "corner": corner}


@pytest.mark.parametrize("which", ["pair", "corner"])
def test_open_and_close_at_the_far_end_of_the_range(dxv, bunny, which):
    """the second half at R = 63 and 64 -- the planes made again from the first half's result, the complement chain; the field form's second
    field of the thresholded grid -- in both forms, restated through distance_sq"""
    vb, ib, _ = bunny
    g = far_halves_grids()[which]
    v = dxv.Voxelizer(0)
    try:
        v.InitFromArrays(vb, ib)
        v.Voxelize(66)
        for r2 in (4095, 4096):
            for op in (mr.OPEN, mr.CLOSE):
                want = mr.morph_by_distance(g, op, r2)
                if (which, op) == ("pair", mr.CLOSE):                   # (OPEN of "corner" is the grid again: its first half is what is not trivial)
                    assert np.count_nonzero(g) < np.count_nonzero(want) < want.size, (which, op, r2)
                for form in (1, 2):
                    v.set_option("morphform", form)
                    check_morph(v, g, lambda: write_grid(v, g), op, r2, want, f"{which}, form {form}")
    finally:
        v.close()


@pytest.mark.parametrize("N", [64, 66, 2])
def test_both_forms_give_the_same_grids_at_small_radii(dxv, bunny, N):
    """the field form below the radius it is picked at: bytes other than 1, N % 8 != 0, every operation"""
    vb, ib, _ = bunny
    v = dxv.Voxelizer(0)
    try:
        v.InitFromArrays(vb, ib)
        v.Voxelize(N)
        for what, g in arbitrary_grids(N):
            for r2 in (1, 10):
                for op in mr.OPS:
                    want = mr.morph(g, op, r2)
                    for form in (2, 1):
                        v.set_option("morphform", form)
                        check_morph(v, g, lambda: write_grid(v, g), op, r2, want, f"N = {N}, {what}, form {form}")
        with pytest.raises(dxv.DxvError, match="morphform"):
            v.set_option("morphform", 3)
    finally:
        v.close()


# ---- the device's own field as second oracle ----------------------------------------------------------------------------------------------
def test_morph_equals_the_threshold_of_the_devices_distance_field(dxv, bunny):
    vb, ib, _ = bunny
    v = dxv.Voxelizer(0)
    try:
        v.InitFromArrays(vb, ib)
        v.Voxelize(128)
        before = v.Grid()
        solid = before != 0
        d = v.DistanceField(dxv.DIST_SQ_I32).astype(np.int64)
        for op, want in ((mr.DILATE, solid | (d <= 9)), (mr.ERODE, solid & (-d > 9))):
            check_morph(v, before, lambda: v.Voxelize(128), op, 9, want.astype(np.uint8), "bunny 128 against the device's field")
        assert 0 < np.count_nonzero(solid & (-d > 9)) < np.count_nonzero(solid)
    finally:
        v.close()


# ---- a large grid against committed hashes ---------------------------------------------------------------------------------------------
def test_morph_of_a_large_grid_equals_committed_hashes(dxv, bunny):
    with open(os.path.join(GOLD, "morph.json")) as fh:
        want = json.load(fh)["bunny/256"]
    vb, ib, _ = bunny
    v = dxv.Voxelizer(0)
    try:
        v.InitFromArrays(vb, ib)
        for op, tag in zip(mr.OPS, ("dilate", "erode", "open", "close")):
            v.Voxelize(256, dxv.MODE_SURFACE)
            assert mr.packed_sha(v.Grid()) == want["grid_packed_sha256"], "the grid is not the one the fixture was made from"
            v.Morph(op, want["radius_sq"])
            assert v.CountSolid() == want[tag]["count"], tag
            assert mr.packed_sha(v.Grid()) == want[tag]["packed_sha256"], f"{tag}: the count agrees but the grid's hash differs"
            assert v.morph_info()[1:] == (want[tag]["set"], want[tag]["cleared"]), tag
    finally:
        v.close()


def test_erode_and_open_of_a_thick_large_grid_equal_committed_hashes(dxv, bunny):
    """the surface at 256^3 erodes to nothing at radius_sq 9; dilated first it is a shell thick enough for ERODE and OPEN to leave something"""
    with open(os.path.join(GOLD, "morph.json")) as fh:
        want = json.load(fh)["bunny/256 thick"]
    vb, ib, _ = bunny
    v = dxv.Voxelizer(0)
    try:
        v.InitFromArrays(vb, ib)
        for op, tag in ((mr.ERODE, "erode"), (mr.OPEN, "open")):
            for form in (1, 2):
                v.set_option("morphform", form)
                v.Voxelize(256, dxv.MODE_SURFACE)
                v.Morph(mr.DILATE, want["thickened_by_radius_sq"])
                assert v.CountSolid() == want["grid_count"] and mr.packed_sha(v.Grid()) == want["grid_packed_sha256"]
                v.Morph(op, want["radius_sq"])
                assert 0 < want[tag]["count"] <= want["grid_count"]
                assert v.CountSolid() == want[tag]["count"], (tag, form)
                assert mr.packed_sha(v.Grid()) == want[tag]["packed_sha256"], f"{tag}, form {form}: the count agrees but the grid's hash differs"
                assert v.morph_info()[1:] == (want[tag]["set"], want[tag]["cleared"]), (tag, form)
    finally:
        v.close()


# ---- the sealing recipe --------------------------------------------------------------------------------------------------------------
def test_dilate_fill_erode_seals_the_holed_shell(dxv, bunny):
    vb, ib, _ = bunny
    holed, whole = mr.holed_shell()
    v = dxv.Voxelizer(0)
    try:
        v.InitFromArrays(vb, ib)
        v.Voxelize(32)
        write_grid(v, holed)
        v.Fill()
        assert v.CountSolid() == 2952                                  # the flood gets in
        write_grid(v, holed)
        v.Morph(dxv.MORPH_DILATE, 8)
        v.Fill()
        v.Morph(dxv.MORPH_ERODE, 8)
        got = v.Grid()
        assert v.CountSolid() == 7208 and np.array_equal(got, fr.fill(whole))
        assert np.array_equal(got, mr.morph(fr.fill(mr.morph(holed, mr.DILATE, 8)), mr.ERODE, 8))
        _, table = v.Components(dxv.COMP_EMPTY, 6)
        assert len(table) == 1                                         # nothing empty is enclosed any more
    finally:
        v.close()


# ---- frame state ---------------------------------------------------------------------------------------------------------------------
def test_three_frames_in_flight_each_get_their_own_morph(dxv, bunny):
    vb, ib, _ = bunny
    v = dxv.Voxelizer(0)
    try:
        v.InitFromArrays(vb, ib)
        plan = [(0, 64, dxv.MODE_REFERENCE, dxv.MORPH_OPEN, 4), (1, 96, dxv.MODE_SURFACE, dxv.MORPH_CLOSE, 9), (2, 48, dxv.MODE_PARITY, dxv.MORPH_ERODE, 2)]
        before = {}
        for frame, N, mode, op, r2 in plan:
            v.Voxelize(N, mode, frameIndex=frame)
            before[frame] = v.Grid()
        for frame, N, mode, op, r2 in plan:                             # no synchronisation between any of these
            v.Voxelize(N, mode, sync=False, frameIndex=frame)
            assert v.Morph(op, r2, sync=False) is True
        v.SyncAll()
        for frame, N, mode, op, r2 in plan:
            v.SetFrame(frame)
            v.Sync()
            want = mr.morph(before[frame], op, r2)
            ms, was_set, cleared = v.morph_info()
            assert ms > 0.0 and (was_set, cleared) == mr.counts(before[frame], want), frame
            got = v.Grid()
            assert got.shape == (N, N, N) and np.array_equal(got, want), frame
    finally:
        v.close()


def test_a_field_and_a_tree_made_before_a_morph_are_stale_after_it(dxv, bunny):
    vb, ib, _ = bunny
    v = dxv.Voxelizer(0)
    try:
        v.InitFromArrays(vb, ib)
        v.Voxelize(64)
        assert v.morph_info() == (0.0, 0, 0)                            # before the first morph
        v.DistanceField(dxv.DIST_SQ_I32)
        v.Octree()
        assert v.distance_device_ptr() and v.OctreeInfo()
        v.Morph(dxv.MORPH_DILATE, 2)
        with pytest.raises(dxv.DxvError, match="stale"):
            v.distance_device_ptr()
        with pytest.raises(dxv.DxvError, match="stale"):
            v.OctreeInfo()
        assert np.array_equal(v.DistanceField(dxv.DIST_SQ_I32), dr.distance_sq(v.Grid()))
    finally:
        v.close()


def test_a_morph_behind_an_unsettled_fill_settles_it_first(dxv, bunny):
    vb, ib, _ = bunny
    v = dxv.Voxelizer(0)
    try:
        v.InitFromArrays(vb, ib)
        v.set_option("fillrounds", 1)                                  # the fill is still unsettled when the morph is asked for
        v.Voxelize(64, dxv.MODE_SURFACE)
        before = v.Grid()
        v.Voxelize(64, dxv.MODE_SURFACE, sync=False)
        assert v.Fill(sync=False) is True
        assert v.Morph(dxv.MORPH_ERODE, 4, sync=False) is True
        v.Sync()
        filled = fr.fill(before)
        assert v.fill_info()[1] > 1
        assert np.array_equal(v.Grid(), mr.morph(filled, mr.ERODE, 4))
    finally:
        v.close()


def test_trim_then_morph_is_the_same(dxv, bunny):
    vb, ib, _ = bunny
    v = dxv.Voxelizer(0)
    try:
        v.InitFromArrays(vb, ib)
        v.Voxelize(64)
        before = v.Grid()
        v.Morph(dxv.MORPH_CLOSE, 9)
        first = v.Grid()
        v.trim()
        assert np.array_equal(v.Grid(), first)                         # the grid stayed
        v.Voxelize(64)
        v.Morph(dxv.MORPH_CLOSE, 9)
        assert np.array_equal(v.Grid(), first) and np.array_equal(first, mr.morph(before, mr.CLOSE, 9))
    finally:
        v.close()


# ---- refusals ------------------------------------------------------------------------------------------------------------------------
def test_morph_refuses_with_a_message_and_launches_nothing(dxv, bunny):
    vb, ib, _ = bunny
    v = dxv.Voxelizer(0)
    lib, ctx = v._lib, v._ctx
    try:
        v.InitFromArrays(vb, ib)
        with pytest.raises(dxv.DxvError, match="no grid yet"):         # before any launch
            v.Morph(dxv.MORPH_DILATE, 1)
        v.Voxelize(64, z0=16, nz=32)
        slab = v.Grid()
        with pytest.raises(dxv.DxvError, match="not a slab or a share"):
            v.Morph(dxv.MORPH_DILATE, 1)
        assert lib.dxv_morph_async(ctx, 0, 1) == 1 and "not a slab or a share" in lib.dxv_last_error(ctx).decode()
        assert np.array_equal(v.Grid(), slab)
        v.VoxelizeInterleaved(64, 1, 2, 8)
        share = v.Grid()
        with pytest.raises(dxv.DxvError, match="not a slab or a share"):
            v.Morph(dxv.MORPH_ERODE, 1)
        assert np.array_equal(v.Grid(), share)
        v.Voxelize(64)
        whole = v.Grid()
        for bad in (4, -1):
            assert lib.dxv_morph_async(ctx, bad, 1) == 1 and "unknown operation" in lib.dxv_last_error(ctx).decode()
            assert lib.dxv_morph(ctx, bad, 1) == 1
        with pytest.raises(dxv.DxvError, match="unknown operation"):
            v.Morph(4, 1)
        for bad in (0, 4097):
            with pytest.raises(dxv.DxvError, match="radius_sq"):
                v.Morph(dxv.MORPH_DILATE, bad)
        assert np.array_equal(v.Grid(), whole)                         # none of the refused calls touched the grid
        assert v.morph_info() == (0.0, 0, 0)
        assert lib.dxv_morph_info(ctx, None, None, None) == 0
        v.Morph(dxv.MORPH_DILATE, 1)
        assert np.array_equal(v.Grid(), mr.morph(whole, mr.DILATE, 1))
    finally:
        v.close()
