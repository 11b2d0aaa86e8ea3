"""The mesh distance field on the GPU (include/dxv.h: dxv_mesh_distance*): the device's field and its nearest triangles equal the numpy
restatement (tests/mesh_distance_restated.py) -- array_equal on the uint32 view, no tolerance -- on the smallest shapes at which the walk
can go wrong, on the asset meshes against committed hashes and samples (tests/golden/mesh_distance.json + mesh_distance_sample.npz, tests/gen_mesh_distance_fixtures.py) and
against the brute-force kernel on the device; the sign is the grid's; slabs, a refitted scene, frame state and refusals."""
import ctypes as C
import hashlib
import json
import os

import numpy as np
import pytest

import mesh_distance_restated as mr
from conftest import GOLD, load_mesh
from raycast_restated import write_grid
from surface_restated import bound_of, normalised_tris

pytestmark = pytest.mark.gpu

NO = np.uint32(mr.NO_TRIANGLE)
BANDS = (0, 3)


@pytest.fixture(scope="module")
def dxv(dxvlib):
    import dxrvoxelizer_amd
    return dxrvoxelizer_amd


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def arrays_of(tris):
    """(vb, ib) of a triangle list (T, 3, 3): private vertices, any normal"""
    pos = np.ascontiguousarray(tris, np.float32).reshape(-1, 3)
    vb = np.ascontiguousarray(np.hstack([pos, np.tile(np.array([[0, 0, 1]], np.float32), (len(pos), 1))]), np.float32)
    return vb, np.arange(len(pos), dtype=np.uint32)


def banded(d2, tri, N, band):
    cap = mr.cap_of(N, band)
    if cap is None:
        return d2, tri
    return np.minimum(d2, cap), np.where(cap < d2, NO, tri).astype(np.uint32)


def check(v, dxv, tris, N, what, z0=0, nz=None):
    """the selected frame's field in both formats, with and without triangles, at band 0 and 3, against the restatement of the
    normalised triangles `tris` signed by the frame's downloaded grid"""
    nz = N if nz is None else nz
    grid = v.Grid().reshape(-1)
    d2, tri = mr.nearest(mr.grid_points(N, z0, nz), tris)
    for band in BANDS:
        b2, btri = banded(d2, tri, N, band)
        for fmt in (dxv.MDIST_VOXELS_F32, dxv.MDIST_UNITS_F32):
            want = mr.value(b2, grid, fmt, N).reshape(nz, N, N)
            for triangles in (False, True):
                got = v.MeshDistanceField(fmt, band, triangles)
                assert got.dtype == np.float32 and got.shape == (nz, N, N), what
                assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (what, band, fmt, triangles)
                if triangles:
                    assert np.array_equal(v.MeshDistanceTriangles().reshape(-1), btri), (what, band, fmt)
                else:
                    with pytest.raises(dxv.DxvError, match="without triangles"):
                        v.MeshDistanceTriangles()
    return grid, d2, tri


# ---- the smallest shapes at which the walk can go wrong ---------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["tetrahedron", "cube"])
@pytest.mark.parametrize("N", [2, 8, 16, 30])                        # 30: no multiple of 4 -- partial bricks; 2: a single partial brick
def test_low_poly_meshes_equal_restatement(dxv, name, N):
    from dxrvoxelizer_amd import meshes
    vb, ib = getattr(meshes, name)()
    v = dxv.Voxelizer(0)
    try:
        v.InitFromArrays(vb, ib)
        v.Voxelize(N)
        grid, d2, _ = check(v, dxv, normalised_tris(vb, ib), N, f"{name} {N}")
        assert N == 2 or grid.any()
    finally:
        v.close()


def test_single_triangle_tree_without_internal_node(dxv):
    tris = np.asarray([[[-0.5, -0.25, 0.1], [0.75, -0.5, -0.2], [0.1, 0.8, 0.3]]], np.float32)
    vb, ib = arrays_of(tris)
    v = dxv.Voxelizer(0)
    try:
        v.InitFromArrays(vb, ib)
        v.Voxelize(8)
        _, _, tri = check(v, dxv, normalised_tris(vb, ib), 8, "one triangle")
        assert (tri == 0).all()
    finally:
        v.close()


@pytest.mark.parametrize("kind", mr.SOUPS)
@pytest.mark.parametrize("N", [16, 24])
def test_soups_equal_restatement(dxv, kind, N):
    vb, ib = arrays_of(mr.soup(kind, 200, 40 + N))
    v = dxv.Voxelizer(0)
    try:
        v.InitFromArrays(vb, ib)
        v.Voxelize(N, dxv.MODE_SURFACE)
        check(v, dxv, normalised_tris(vb, ib), N, f"{kind} {N}")
    finally:
        v.close()


def test_two_coincident_cubes_take_the_smaller_index(dxv):
    from dxrvoxelizer_amd import meshes
    vb, ib = meshes.cube()
    vb2, ib2 = np.concatenate([vb, vb]), np.concatenate([ib, ib + len(vb)]).astype(np.uint32)
    v = dxv.Voxelizer(0)
    try:
        v.InitFromArrays(vb2, ib2)
        v.Voxelize(16)
        _, _, tri = check(v, dxv, normalised_tris(vb2, ib2), 16, "two cubes")
        assert (tri < 12).all()                                       # every minimum is reached by a triangle of either copy: the first one's
    finally:
        v.close()


# ---- assets ----------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def golden():
    with open(os.path.join(GOLD, "mesh_distance.json")) as fh:
        return json.load(fh)


@pytest.fixture(scope="module")
def golden_sample():
    return np.load(os.path.join(GOLD, "mesh_distance_sample.npz"))


@pytest.mark.parametrize("name", ["bunny", "dragon", "turingbowl"])
def test_assets_at_32_equal_committed_fixture(dxv, golden, golden_sample, name):
    N = 32
    fix = golden[f"{name}/{N}"]
    vb, ib, _ = load_mesh(name)
    assert fix["triangles"] == len(ib) // 3
    v = dxv.Voxelizer(0)
    try:
        v.InitFromArrays(vb, ib)
        for mode in (dxv.MODE_REFERENCE, dxv.MODE_SURFACE):           # the sign follows the grid, the magnitude does not
            v.Voxelize(N, mode)
            solid = v.Grid() != 0
            assert solid.any() and not solid.all()
            for band in BANDS:
                want = fix[f"band{band}"]
                where = np.sort(np.random.default_rng(fix["sample"]["seed"]).choice(N ** 3, fix["sample"]["voxels"], replace=False))
                bits, tris = golden_sample[f"{name}_band{band}_bits"], golden_sample[f"{name}_band{band}_tri"]
                assert len(bits) == len(tris) == 4096
                for fmt, key in ((dxv.MDIST_VOXELS_F32, "voxels"), (dxv.MDIST_UNITS_F32, "units")):
                    got = v.MeshDistanceField(fmt, band, True)
                    tri = v.MeshDistanceTriangles()
                    assert np.array_equal(np.signbit(got), solid), (name, mode, band, key)
                    mag = np.abs(got)
                    if fmt == dxv.MDIST_VOXELS_F32:
                        assert np.array_equal(mag.reshape(-1)[where].view(np.uint32), bits), (name, mode, band)
                    assert np.array_equal(tri.reshape(-1)[where], tris), (name, mode, band)
                    w = want[key]
                    assert (float(mag.min()).hex(), float(mag.max()).hex(), float(mag.sum(dtype=np.float64)).hex()) == (w["min"], w["max"], w["sum"])
                    assert sha(mag) == w["sha256"], (name, mode, band, key)
                    assert sha(tri) == want["tri_sha256"], (name, mode, band, key)
    finally:
        v.close()


def test_bunny_at_64_walk_equals_brute_force_kernel(dxv, bunny):
    vb, ib, _ = bunny
    v = dxv.Voxelizer(0)
    try:
        v.InitFromArrays(vb, ib)
        for mode in (dxv.MODE_REFERENCE, dxv.MODE_SURFACE):
            v.Voxelize(64, mode)
            for band in BANDS:
                v.set_option("mdistwalk", 1)
                walk = v.MeshDistanceField(dxv.MDIST_UNITS_F32, band, True)
                wtri = v.MeshDistanceTriangles()
                v.set_option("mdistwalk", 0)
                brute = v.MeshDistanceField(dxv.MDIST_UNITS_F32, band, True)
                btri = v.MeshDistanceTriangles()
                assert np.array_equal(walk.view(np.uint32), brute.view(np.uint32)) and np.array_equal(wtri, btri), (mode, band)
                assert np.array_equal(np.signbit(walk), v.Grid() != 0)
                assert (wtri == NO).any() == (band != 0) and (wtri != NO).any()
    finally:
        v.close()


# ---- the sign is the grid's ------------------------------------------------------------------------------------------------------
def test_sign_follows_a_written_grid_and_magnitudes_stay(dxv):
    from dxrvoxelizer_amd import meshes
    vb, ib = meshes.cube()
    N = 16
    v = dxv.Voxelizer(0)
    try:
        v.InitFromArrays(vb, ib)
        v.Voxelize(N)
        before = v.MeshDistanceField(dxv.MDIST_VOXELS_F32)
        rng = np.random.default_rng(3)
        g = ((rng.random((N, N, N)) < 0.5) * rng.integers(1, 256, (N, N, N))).astype(np.uint8)     # (any non-zero byte is solid)
        write_grid(v, g)
        after = v.MeshDistanceField(dxv.MDIST_VOXELS_F32)
        assert np.array_equal(np.abs(after).view(np.uint32), np.abs(before).view(np.uint32))
        assert np.array_equal(np.signbit(after), g != 0)
    finally:
        v.close()


# ---- partitions ------------------------------------------------------------------------------------------------------------------
def test_slab_equals_those_slices_and_a_share_is_refused(dxv, bunny):
    vb, ib, _ = bunny
    N = 64
    v = dxv.Voxelizer(0)
    try:
        v.InitFromArrays(vb, ib)
        v.Voxelize(N)
        whole = v.MeshDistanceField(dxv.MDIST_UNITS_F32, 0, True)
        wtri = v.MeshDistanceTriangles()
        v.Voxelize(N, z0=16, nz=32)
        slab = v.MeshDistanceField(dxv.MDIST_UNITS_F32, 0, True)
        assert slab.shape == (32, N, N) and v._lib.dxv_mesh_distance_bytes(v._ctx) == 4 * 32 * N * N
        assert np.array_equal(slab.view(np.uint32), whole[16:48].view(np.uint32))
        assert np.array_equal(v.MeshDistanceTriangles(), wtri[16:48])
        v.VoxelizeInterleaved(N, 1, 2, 8)
        with pytest.raises(dxv.DxvError, match="interleaved share"):
            v.MeshDistanceField()
        assert v._lib.dxv_mesh_distance_device_ptr(v._ctx) is None and v._lib.dxv_mesh_distance_bytes(v._ctx) == 0
    finally:
        v.close()


# ---- a dynamic scene -------------------------------------------------------------------------------------------------------------
def test_refitted_scene_with_deferred_boxes_equals_restatement_of_new_positions(dxv, bunny):
    vb, ib, _ = bunny
    ib = np.ascontiguousarray(ib.reshape(-1, 3)[::35].reshape(-1))    # a decimated subset: 1 991 triangles
    assert len(ib) // 3 <= 2000
    bound = bound_of(vb)
    v = dxv.Voxelizer(0)
    try:
        v.InitDynamic(vb, ib)
        v.Voxelize(16)
        v.Voxelize(16)                                                 # (the scene has lists now: the refit defers the node boxes)
        moved = vb.copy()
        moved[:, :3] = (moved[:, :3] - moved[:, :3].mean(0)) * np.float32(0.7) + moved[:, :3].mean(0)
        v.UpdateVertices(moved)                                        # update_vertices + refit, default deferboxes: the bound of Init stays
        v.Voxelize(16)
        check(v, dxv, normalised_tris(moved, ib, bound), 16, "refitted bunny subset")
    finally:
        v.close()


def test_refit_waits_for_a_field_still_in_flight_on_another_frame(dxv, bunny):
    """frame 1 synchronised, its field enqueued without a wait, then a refit: the field is the OLD positions', the next one the new ones'"""
    vb, ib, _ = bunny
    moved = vb.copy()
    moved[:, :3] = (moved[:, :3] - moved[:, :3].mean(0)) * np.float32(0.7) + moved[:, :3].mean(0)
    sub = np.ascontiguousarray(ib.reshape(-1, 3)[::35].reshape(-1))   # 1 991 triangles: against the restatement at 16^3
    bound = bound_of(vb)
    for indices, N, restate in ((sub, 16, True), (ib, 128, False)):   # ... and the whole bunny at 128^3, a walk of milliseconds, against the waited-for field
        v = dxv.Voxelizer(0)
        try:
            v.InitDynamic(vb, indices)
            v.Voxelize(N, frameIndex=1)                                # synchronised: nothing of the launch is pending
            ref, rtri = (None, None) if restate else (v.MeshDistanceField(dxv.MDIST_UNITS_F32, 0, True), v.MeshDistanceTriangles())
            grid = v.Grid().reshape(-1)
            assert v.MeshDistanceField(dxv.MDIST_UNITS_F32, 0, True, sync=False) is True
            v.UpdateVertices(moved)                                    # upload + refit on the context's stream, frame 1 still selected
            v.Sync()
            got, gtri = v.MeshDistance(), v.MeshDistanceTriangles()
            if restate:
                d2, tri = mr.nearest(mr.grid_points(N), normalised_tris(vb, indices, bound))
                ref, rtri = mr.value(d2, grid, dxv.MDIST_UNITS_F32, N).reshape(N, N, N), tri.reshape(N, N, N)
            assert np.array_equal(got.view(np.uint32), ref.view(np.uint32)) and np.array_equal(gtri, rtri), N
            if restate:                                                # the next field is the new positions'
                d2, tri = mr.nearest(mr.grid_points(N), normalised_tris(moved, indices, bound))
                new = v.MeshDistanceField(dxv.MDIST_UNITS_F32, 0, True)
                assert np.array_equal(np.abs(new).view(np.uint32), mr.value(d2, np.zeros(N ** 3, np.uint8), dxv.MDIST_UNITS_F32, N).reshape(N, N, N).view(np.uint32))
                assert np.array_equal(v.MeshDistanceTriangles().reshape(-1), tri)
        finally:
            v.close()


# ---- frame state, refusals -------------------------------------------------------------------------------------------------------
def test_field_is_stale_after_voxelize_and_after_fill_and_trim_keeps_it(dxv):
    from dxrvoxelizer_amd import meshes
    vb, ib = meshes.cube()
    v = dxv.Voxelizer(0)
    lib, ctx = v._lib, v._ctx
    try:
        v.InitFromArrays(vb, ib)
        v.Voxelize(16, dxv.MODE_SURFACE)
        first = v.MeshDistanceField(dxv.MDIST_VOXELS_F32, 0, True)
        ftri = v.MeshDistanceTriangles()
        assert lib.dxv_mesh_distance_bytes(ctx) == 4 * 16 ** 3 and v.mesh_distance_device_ptr() and lib.dxv_mesh_distance_triangles_device_ptr(ctx)
        assert v.mesh_distance_ms() > 0.0
        v.trim()                                                       # the field stays
        assert np.array_equal(v.MeshDistance().view(np.uint32), first.view(np.uint32)) and np.array_equal(v.MeshDistanceTriangles(), ftri)
        v.Fill(dxv.FILL_INTERIOR)                                      # the grid changed under the field
        with pytest.raises(dxv.DxvError, match="stale"):
            v.mesh_distance_device_ptr()
        assert lib.dxv_mesh_distance_bytes(ctx) == 0 and lib.dxv_mesh_distance_triangles_device_ptr(ctx) is None
        filled = v.MeshDistanceField(dxv.MDIST_VOXELS_F32)            # Voxelize(SURFACE); Fill(INTERIOR); MeshDistanceField(): negative inside
        assert np.array_equal(np.abs(filled).view(np.uint32), np.abs(first).view(np.uint32))
        assert np.array_equal(np.signbit(filled), v.Grid() != 0) and np.signbit(filled).any()
        v.Voxelize(16)                                                 # launched again
        buf = np.empty(16 ** 3, np.float32)
        assert lib.dxv_mesh_distance_download(ctx, buf.ctypes.data_as(C.c_void_p), buf.nbytes) == 1 and "stale" in lib.dxv_last_error(ctx).decode()
        assert lib.dxv_mesh_distance_triangles_download(ctx, buf.ctypes.data_as(C.c_void_p), buf.nbytes) == 1
    finally:
        v.close()


def test_three_frames_in_flight_each_get_their_own_field(dxv, bunny):
    vb, ib, _ = bunny
    ib = np.ascontiguousarray(ib.reshape(-1, 3)[::70].reshape(-1))    # 996 triangles: the restatement of three small grids stays quick
    tris = normalised_tris(vb, ib)
    v = dxv.Voxelizer(0)
    try:
        v.InitFromArrays(vb, ib)
        plan = [(0, 16, dxv.MODE_REFERENCE, dxv.MDIST_VOXELS_F32, 0), (1, 24, dxv.MODE_SURFACE, dxv.MDIST_UNITS_F32, 3),
                (2, 12, dxv.MODE_REFERENCE_SURFACE, dxv.MDIST_VOXELS_F32, 2)]
        for frame, N, mode, fmt, band in plan:                         # no synchronisation between any of these
            v.Voxelize(N, mode, sync=False, frameIndex=frame)
            assert v.MeshDistanceField(fmt, band, True, sync=False) is True
        v.SyncAll()
        for frame, N, mode, fmt, band in plan:
            v.SetFrame(frame)
            v.Sync()
            assert v.mesh_distance_ms() > 0.0, frame
            d2, tri = banded(*mr.nearest(mr.grid_points(N), tris), N, band)
            got = v.MeshDistance()
            assert got.shape == (N, N, N)
            assert np.array_equal(got.view(np.uint32), mr.value(d2, v.Grid().reshape(-1), fmt, N).reshape(N, N, N).view(np.uint32)), frame
            assert np.array_equal(v.MeshDistanceTriangles().reshape(-1), tri), frame
    finally:
        v.close()


def test_mesh_distance_refuses_with_a_message_and_launches_nothing(dxv):
    from dxrvoxelizer_amd import meshes
    vb, ib = meshes.cube()
    v = dxv.Voxelizer(0)
    lib, ctx = v._lib, v._ctx

    def nothing():
        return lib.dxv_mesh_distance_device_ptr(ctx) is None and lib.dxv_mesh_distance_bytes(ctx) == 0

    try:
        assert lib.dxv_mesh_distance_async(ctx, 0, 0, 0) == 1 and "no grid yet" in lib.dxv_last_error(ctx).decode()   # no scene, no grid
        v.InitFromArrays(vb, ib)
        with pytest.raises(dxv.DxvError, match="no grid yet"):
            v.MeshDistanceField()
        assert nothing()
        v.Voxelize(16)
        for bad in (-1, 2, 7):
            assert lib.dxv_mesh_distance_async(ctx, bad, 0, 0) == 1 and "unknown format" in lib.dxv_last_error(ctx).decode()
            assert lib.dxv_mesh_distance(ctx, bad, 0, 0) == 1
        with pytest.raises(dxv.DxvError, match="unknown format"):
            v.MeshDistanceField(format=5)
        assert lib.dxv_mesh_distance_async(ctx, 0, 4097, 0) == 1 and "band" in lib.dxv_last_error(ctx).decode()
        v.VoxelizeInterleaved(16, 0, 2, 4)
        assert lib.dxv_mesh_distance_async(ctx, 0, 0, 1) == 1 and "interleaved share" in lib.dxv_last_error(ctx).decode()
        assert nothing()                                               # nothing was launched by any of those
        v.Voxelize(16)
        vbc, ibc = np.ascontiguousarray(vb, np.float32).reshape(-1, 6), np.ascontiguousarray(ib, np.uint32).reshape(-1)
        assert lib.dxv_set_mesh(ctx, vbc, len(vbc), ibc, ibc.size // 3) == 0                     # a grid, a mesh, but no built hierarchy
        assert lib.dxv_mesh_distance_async(ctx, 0, 0, 0) == 1 and "no scene with a built hierarchy" in lib.dxv_last_error(ctx).decode()
        assert lib.dxv_mesh_distance(ctx, 1, 3, 1) == 1 and nothing()
        assert lib.dxv_build(ctx) == 0
        v.Voxelize(16)
        f = v.MeshDistanceField(dxv.MDIST_UNITS_F32, 4096)             # the largest band is accepted
        buf = np.empty(16 ** 3 + 1, np.float32)
        assert lib.dxv_mesh_distance_download(ctx, buf.ctypes.data_as(C.c_void_p), buf.nbytes) == 1
        assert "expected 16384 bytes" in lib.dxv_last_error(ctx).decode()
        assert lib.dxv_mesh_distance_download(ctx, None, 4 * 16 ** 3) == 1
        assert lib.dxv_mesh_distance_triangles_download(ctx, buf.ctypes.data_as(C.c_void_p), 4 * 16 ** 3) == 1
        assert "without triangles" in lib.dxv_last_error(ctx).decode()
        assert lib.dxv_mesh_distance_ms(ctx, None) == 1
        assert np.isfinite(f).all()
    finally:
        v.close()
