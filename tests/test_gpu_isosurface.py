"""Isosurface extraction on the GPU (include/dxv.h: dxv_isosurface*): the device's vertex and index buffers equal the numpy restatement
(tests/isosurface_restated.py) of the field they were made from byte for byte -- low-poly meshes through the mesh distance field in both
formats, arbitrary grids written through the frame's grid pointer through the grid distance field, three levels, both spaces, grids whose
cell rows end inside a word and grids whose rows need two --, the remesh of the bunny is closed and goes back through Init to the same
solid, three frames extract side by side, and the calls refuse what they must.
Not covered here: the refusal of a mesh over 2^31 - 1 vertices or index words, which needs a field of tens of gigabytes."""
import ctypes as C

import numpy as np
import pytest

import isosurface_restated as ir
from raycast_restated import write_grid

pytestmark = pytest.mark.gpu

F32 = np.float32


@pytest.fixture(scope="module")
def dxv(dxvlib):
    import dxrvoxelizer_amd
    return dxrvoxelizer_amd


def field_of(v, dxv, source):
    return v.MeshDistance() if source == dxv.ISO_MESH_DISTANCE else v.Distance()


def check(v, dxv, source, iso, P, space, what):
    """the selected frame's mesh of (source, iso, space) against the restatement of the frame's downloaded field; returns it"""
    vb, ib = v.Isosurface(source, float(iso), space)
    field = field_of(v, dxv, source)
    assert field.dtype == F32
    wv, wi = ir.extract(field, iso, P, space, np.asarray(v.stats()["bound"], F32))
    assert vb.shape == wv.shape and ib.shape == wi.shape, (what, vb.shape, wv.shape, ib.shape, wi.shape)
    assert v.IsosurfaceCounts() == (len(wv), len(wi) // 3), what
    assert np.array_equal(vb.view(np.uint32), wv.view(np.uint32)), what
    assert ib.dtype == np.uint32 and np.array_equal(ib, wi), what
    pv, pi = v.isosurface_device_ptrs()
    assert (pv is not None) == (len(wv) > 0) and (pi is not None) == (len(wi) > 0), what
    return vb, ib


def all_levels_and_spaces(v, dxv, source, P, what):
    n = 0
    for k in (0.0, 0.5, -0.5):
        for space in (dxv.ISO_SPACE_VOXELS, dxv.ISO_SPACE_OBJECT):
            vb, ib = check(v, dxv, source, F32(k) * F32(P), P, space, f"{what}, iso {k} P, space {space}")
            assert ir.directed_edges_pair_up(ib), what
            n += len(ib)
    return n


@pytest.mark.parametrize("N", [2, 8, 16, 30])                          # 30 and 2: rows of 31 and 3 cells, part of a word
@pytest.mark.parametrize("name", ["tetrahedron", "cube"])
def test_low_poly_meshes_through_the_mesh_distance_field_equal_restatement(dxv, name, N):
    from dxrvoxelizer_amd import meshes
    vb, ib = getattr(meshes, name)()
    v = dxv.Voxelizer(0)
    try:
        v.InitFromArrays(vb, ib)
        v.Voxelize(N, dxv.MODE_PARITY)
        assert v.Grid().any()
        for fmt in (dxv.MDIST_VOXELS_F32, dxv.MDIST_UNITS_F32):
            v.MeshDistanceField(fmt)
            assert all_levels_and_spaces(v, dxv, dxv.ISO_MESH_DISTANCE, ir.voxel(N, fmt == dxv.MDIST_UNITS_F32), f"{name} {N} format {fmt}") > 0
    finally:
        v.close()


def written_grids():
    rng = np.random.default_rng(7)
    for N in (8, 16):
        yield f"random {N}", (rng.random((N, N, N)) < 0.5).astype(np.uint8)
    z, y, x = np.indices((8, 8, 8))
    yield "checkerboard 8", ((x + y + z) & 1).astype(np.uint8)
    yield "all solid 8", np.full((8, 8, 8), 0xFF, np.uint8)
    yield "all empty 8", np.zeros((8, 8, 8), np.uint8)
    one = np.zeros((8, 8, 8), np.uint8)
    one[7, 0, 3] = 1
    yield "one voxel 8", one
    slab = np.zeros((66, 66, 66), np.uint8)                             # a cell row of 67 cells: two words, the solid runs through the boundary
    slab[30:34, 20:23, 3:66] = 1
    yield "slab 66", slab


GRIDS = list(written_grids())


@pytest.fixture(scope="module")
def writer(dxv, bunny):
    vb, ib, _ = bunny
    v = dxv.Voxelizer(0)
    v.InitFromArrays(vb, ib)
    yield v
    v.close()


@pytest.mark.parametrize("case", GRIDS, ids=[g[0] for g in GRIDS])
def test_written_grids_through_the_grid_distance_field_equal_restatement(dxv, writer, case):
    what, g = case
    v = writer
    v.Voxelize(g.shape[0])
    write_grid(v, g)
    v.DistanceField(dxv.DIST_F32)
    n = all_levels_and_spaces(v, dxv, dxv.ISO_GRID_DISTANCE, F32(1.0), what)
    assert (n > 0) == bool(g.any())
    if what == "all empty 8":                                          # the empty mesh is a success: zero counts, no pointers, downloads of nothing
        assert v.IsosurfaceCounts() == (0, 0) and v.isosurface_device_ptrs() == (None, None)
        assert v._lib.dxv_isosurface_vertices_download(v._ctx, None, 0) == 0 and v._lib.dxv_isosurface_indices_download(v._ctx, None, 0) == 0
    if what == "all solid 8":                                          # -INF inside: every crossing at one half, the box of the whole grid
        vb, ib = v.Isosurface(dxv.ISO_GRID_DISTANCE, 0.0, dxv.ISO_SPACE_VOXELS)
        assert 7 ** 3 <= ir.signed_volume(vb, ib) <= 8 ** 3 and (vb[:, 3:] == 0).all()      # (the nets only cut the corners; Inf differences: no normal)


def test_remesh_of_the_leaky_recipe_equals_restatement_and_is_closed(dxv, bunny):
    vb, ib, _ = bunny
    v = dxv.Voxelizer(0)
    try:
        v.InitFromArrays(vb, ib)
        v.Voxelize(32, dxv.MODE_SURFACE)
        v.Fill(dxv.FILL_INTERIOR)
        v.MeshDistanceField()
        for space in (dxv.ISO_SPACE_OBJECT, dxv.ISO_SPACE_VOXELS):
            mv, mi = check(v, dxv, dxv.ISO_MESH_DISTANCE, 0.0, F32(1.0), space, f"bunny 32, space {space}")
            assert len(mi) > 0 and ir.directed_edges_pair_up(mi) and ir.signed_volume(mv, mi) > 0.0
        assert v.isosurface_ms() > 0.0
    finally:
        v.close()


def test_round_trip_through_init_gives_the_same_solid_away_from_the_surface(dxv, bunny):
    vb, ib, _ = bunny
    N = 32
    v, w = dxv.Voxelizer(0), dxv.Voxelizer(0)
    try:
        v.InitFromArrays(vb, ib)
        v.Voxelize(N)
        grid = v.Grid()
        d = v.DistanceField(dxv.DIST_F32)
        mv, mi = v.Isosurface(dxv.ISO_GRID_DISTANCE, 0.0, dxv.ISO_SPACE_OBJECT)
        w.InitFromArrays(mv, mi)
        w.Voxelize(N, dxv.MODE_PARITY)
        again = w.Grid()
        b0, b1 = np.asarray(v.stats()["bound"], np.float64), np.asarray(w.stats()["bound"], np.float64)
        shift = (np.abs(b1[:3] - b0[:3]).max() + abs(b1[3] - b0[3])) / b0[3] * N / 2
        far = np.abs(d) >= 2                                           # no active cell touches such a voxel: every corner within sqrt(3) of it is of its kind
        wrong = int(((grid != 0) != (again != 0))[far].sum())
        print(f"round trip: {len(mv)} vertices, {len(mi) // 3} triangles, bound shift {shift:.4f} voxels, {int(far.sum())} voxels compared, {wrong} differ")
        assert far.any() and (grid[far] != 0).any() and (grid[far] == 0).any()
        assert wrong == 0
    finally:
        v.close()
        w.close()


def test_three_frames_in_flight_each_get_their_own_mesh(dxv, bunny):
    vb, ib, _ = bunny
    v = dxv.Voxelizer(0)
    try:
        v.InitFromArrays(vb, ib)
        plan = [(0, 16, dxv.ISO_MESH_DISTANCE, dxv.MDIST_VOXELS_F32, 0.0, dxv.ISO_SPACE_OBJECT),
                (1, 24, dxv.ISO_GRID_DISTANCE, None, 0.5, dxv.ISO_SPACE_VOXELS),
                (2, 12, dxv.ISO_MESH_DISTANCE, dxv.MDIST_UNITS_F32, -0.5 * 2 / 12, dxv.ISO_SPACE_OBJECT)]
        for frame, N, source, fmt, iso, space in plan:                 # no synchronisation between any of these
            v.Voxelize(N, sync=False, frameIndex=frame)
            if source == dxv.ISO_MESH_DISTANCE:
                assert v.MeshDistanceField(fmt, sync=False) is True
            else:
                assert v.DistanceField(dxv.DIST_F32, sync=False) is True
            assert v.Isosurface(source, iso, space, sync=False) is True
        v.SyncAll()
        seen = set()
        for frame, N, source, fmt, iso, space in plan:
            v.SetFrame(frame)
            v.Sync()
            assert v.isosurface_ms() > 0.0, frame
            P = ir.voxel(N, fmt == dxv.MDIST_UNITS_F32)
            wv, wi = ir.extract(field_of(v, dxv, source), iso, P, space, np.asarray(v.stats()["bound"], F32))
            gv, gi = v.IsosurfaceMesh()
            assert gv.shape == wv.shape and np.array_equal(gv.view(np.uint32), wv.view(np.uint32)) and np.array_equal(gi, wi), frame
            assert len(wi) > 0
            seen.add(v.isosurface_device_ptrs())
        assert len(seen) == 3
    finally:
        v.close()


def test_mesh_is_stale_after_voxelize_and_after_fill_and_trim_keeps_it(dxv):
    from dxrvoxelizer_amd import meshes
    vb, ib = meshes.cube()
    v = dxv.Voxelizer(0)
    lib, ctx = v._lib, v._ctx
    try:
        v.InitFromArrays(vb, ib)
        v.Voxelize(16, dxv.MODE_SURFACE)
        v.MeshDistanceField()
        first = v.Isosurface(dxv.ISO_MESH_DISTANCE, 1.0, dxv.ISO_SPACE_OBJECT)     # the offset surface one voxel outside the shell
        assert len(first[1]) > 0
        v.trim()                                                       # the scratch goes, the mesh stays
        again = v.IsosurfaceMesh()
        assert np.array_equal(again[0].view(np.uint32), first[0].view(np.uint32)) and np.array_equal(again[1], first[1])
        after = v.Isosurface(dxv.ISO_MESH_DISTANCE, 1.0, dxv.ISO_SPACE_OBJECT)     # ... and the next extraction is the same mesh
        assert np.array_equal(after[0].view(np.uint32), first[0].view(np.uint32)) and np.array_equal(after[1], first[1])
        v.Fill(dxv.FILL_INTERIOR)                                      # the grid changed under the mesh
        with pytest.raises(dxv.DxvError, match="stale"):
            v.IsosurfaceCounts()
        assert lib.dxv_isosurface_vertices_device_ptr(ctx) is None and "stale" in lib.dxv_last_error(ctx).decode()
        assert lib.dxv_isosurface_indices_device_ptr(ctx) is None
        buf = np.empty_like(first[0])
        assert lib.dxv_isosurface_vertices_download(ctx, buf.ctypes.data_as(C.c_void_p), buf.nbytes) == 1 and "stale" in lib.dxv_last_error(ctx).decode()
        with pytest.raises(dxv.DxvError, match="stale"):                # ... and under its field
            v.Isosurface(dxv.ISO_MESH_DISTANCE)
        v.MeshDistanceField()
        v.Isosurface(dxv.ISO_MESH_DISTANCE)
        assert v.IsosurfaceCounts()[0] > 0
        v.Voxelize(16)                                                 # launched again
        with pytest.raises(dxv.DxvError, match="stale"):
            v.IsosurfaceMesh()
        ibuf = np.empty(3, np.uint32)
        assert lib.dxv_isosurface_indices_download(ctx, ibuf.ctypes.data_as(C.c_void_p), ibuf.nbytes) == 1 and "stale" in lib.dxv_last_error(ctx).decode()
    finally:
        v.close()


def test_isosurface_refuses_with_a_message_and_launches_nothing(dxv):
    from dxrvoxelizer_amd import meshes
    vb, ib = meshes.cube()
    v = dxv.Voxelizer(0)
    lib, ctx = v._lib, v._ctx

    def refused(source, iso, space, text):
        for fn in (lib.dxv_isosurface_async, lib.dxv_isosurface):
            assert fn(ctx, source, iso, space) == 1 and text in lib.dxv_last_error(ctx).decode(), (text, lib.dxv_last_error(ctx).decode())
        assert lib.dxv_isosurface_counts(ctx, None, None) == 1 and "no isosurface yet" in lib.dxv_last_error(ctx).decode()   # nothing was made
        assert lib.dxv_isosurface_vertices_device_ptr(ctx) is None and lib.dxv_isosurface_indices_device_ptr(ctx) is None

    try:
        refused(0, 0.0, 0, "no mesh distance field yet")               # no scene, no grid
        refused(1, 0.0, 0, "no distance field yet")
        v.InitFromArrays(vb, ib)
        v.Voxelize(16)
        refused(0, 0.0, 1, "no mesh distance field yet")
        v.MeshDistanceField()
        v.DistanceField(dxv.DIST_SQ_I32)
        for bad in (-1, 2, 9):
            refused(bad, 0.0, 0, "unknown source")
            refused(0, 0.0, bad, "unknown space")
        with pytest.raises(dxv.DxvError, match="unknown source"):
            v.Isosurface(source=3)
        with pytest.raises(dxv.DxvError, match="unknown space"):
            v.Isosurface(space=3)
        for bad in (np.nan, np.inf, -np.inf):
            refused(0, bad, 0, "iso must be finite")
        refused(1, 0.0, 0, "int32 format")
        v.Voxelize(16)                                                 # both fields are stale now
        refused(0, 0.0, 0, "stale")
        refused(1, 0.0, 0, "stale")
        v.Voxelize(16, z0=4, nz=8)
        v.MeshDistanceField()                                          # a slab's field: fine for the field, not for the lattice
        refused(0, 0.0, 0, "slab")
        v.Voxelize(16)
        v.MeshDistanceField()
        v.DistanceField(dxv.DIST_F32)
        vbc, ibc = np.ascontiguousarray(vb, np.float32).reshape(-1, 6), np.ascontiguousarray(ib, np.uint32).reshape(-1)
        assert lib.dxv_set_mesh(ctx, vbc, len(vbc), ibc, ibc.size // 3) == 0                     # fields, a mesh, but no scene
        refused(0, 0.0, 1, "no scene")
        refused(1, 0.0, 1, "no scene")
        assert lib.dxv_isosurface(ctx, 1, 0.0, 0) == 0                 # voxel space needs no bound
        nv, nt = v.IsosurfaceCounts()
        assert nv > 0 and nt > 0
        buf = np.empty((nv + 1, 6), np.float32)
        assert lib.dxv_isosurface_vertices_download(ctx, buf.ctypes.data_as(C.c_void_p), buf.nbytes) == 1
        assert f"expected {24 * nv} bytes" in lib.dxv_last_error(ctx).decode()
        assert lib.dxv_isosurface_vertices_download(ctx, None, 24 * nv) == 1
        assert lib.dxv_isosurface_indices_download(ctx, buf.ctypes.data_as(C.c_void_p), 12 * nt + 4) == 1
        assert f"expected {12 * nt} bytes" in lib.dxv_last_error(ctx).decode()
        assert lib.dxv_isosurface_ms(ctx, None) == 1
    finally:
        v.close()
