"""The distance field on the GPU (include/dxv.h: dxv_distance*): every voxel of the device's field equals the numpy restatement
(tests/distance_restated.py) of the grid the field was made from -- array_equal, no tolerance, both formats -- for meshes in every mode,
for arbitrary grids written through the frame's grid pointer, for large grids against committed hashes (tests/golden/distance.json,
tests/gen_distance_fixtures.py), for three frames in flight; and the calls refuse what they must."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import distance_restated as dr
from conftest import GOLD, load_mesh
from raycast_restated import write_grid
from test_gpu_configs import make, sha

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dxv(dxvlib):
    import dxrvoxelizer_amd
    return dxrvoxelizer_amd


def check_field(v, dxv, what):
    """both formats of the selected frame's field against the restatement of the frame's downloaded grid"""
    grid = v.Grid()
    want = dr.distance_sq(grid)
    got = v.DistanceField(dxv.DIST_SQ_I32)
    assert got.dtype == np.int32 and np.array_equal(got, want), what
    f = v.DistanceField(dxv.DIST_F32)
    mag = np.abs(want.astype(np.int64))
    root = np.where(mag == dr.NONE, np.float32(np.inf), np.sqrt(mag.astype(np.float32))).astype(np.float32)
    assert f.dtype == np.float32 and np.array_equal(f, np.where(want < 0, -root, root)), what
    assert np.array_equal(f.view(np.uint32), dr.to_f32(want).view(np.uint32)), what
    return grid, want


@pytest.mark.parametrize("name,N,modes", [("bunny", 64, (0, 1, 2, 3)), ("dragon", 64, (0, 1, 2, 3)), ("turingbowl", 64, (0, 1, 2, 3)),
                                          ("bunny", 128, (0, 3))])
def test_field_of_mesh_grids_equals_restatement(dxv, name, N, modes):
    vb, ib, _ = load_mesh(name)
    v = dxv.Voxelizer(0)
    try:
        v.InitFromArrays(vb, ib)
        for mode in modes:
            v.Voxelize(N, mode)
            grid, want = check_field(v, dxv, f"{name} {N} mode {mode}")
            assert grid.any() and (want < 0).any() and (want > 0).any()
    finally:
        v.close()


def arbitrary_grids(N):
    rng = np.random.default_rng(N)
    z, y, x = np.indices((N, N, N))
    for density in (0.5, 0.01, 1e-4):
        g = ((rng.random((N, N, N)) < density) * rng.integers(1, 256, (N, N, N))).astype(np.uint8)   # (bytes other than 0 / 1 are solid too)
        if density == 1e-4 and not g.any():
            g[N // 3, N // 2, N - 1] = 77
        yield f"random {density}", g
    yield "all zero", np.zeros((N, N, N), np.uint8)
    yield "all 0xFF", np.full((N, N, N), 0xFF, np.uint8)
    one = np.zeros((N, N, N), np.uint8)
    one[N - 1, 0, N // 2] = 1
    yield "one voxel", one
    yield "checkerboard", ((x + y + z) & 1).astype(np.uint8)


@pytest.mark.parametrize("N", [64, 96, 2])                           # 96: no power of two, rows of one and a half words; 2: the smallest grid
def test_field_of_arbitrary_grids_equals_restatement(dxv, bunny, N):
    vb, ib, _ = bunny
    v = dxv.Voxelizer(0)
    try:
        v.InitFromArrays(vb, ib)
        v.Voxelize(N)
        for what, g in arbitrary_grids(N):
            write_grid(v, g)
            grid, _ = check_field(v, dxv, f"N = {N}, {what}")
            assert np.array_equal(grid, g)
    finally:
        v.close()


@pytest.mark.parametrize("key", ["bunny/256", "torus1m/512", "dragon9/512"])
def test_field_of_large_grids_equals_committed_hashes(dxv, key):
    with open(os.path.join(GOLD, "distance.json")) as fh:
        want = json.load(fh)[key]
    name, N = key.split("/")
    vb, ib = make(name)
    v = dxv.Voxelizer(0)
    try:
        v.InitFromArrays(vb, ib)
        v.Voxelize(int(N))
        assert sha(v.Grid()) == want["grid_sha256"], f"{key}: the grid is not the one the fixture's field was made from"
        f = v.DistanceField(dxv.DIST_SQ_I32)
        assert (int(f.min()), int(f.max()), int(f.sum(dtype=np.int64))) == (want["min"], want["max"], want["sum"]), key
        assert sha(f) == want["sha256"], f"{key}: min, max and sum agree but the field's hash differs"
        r = v.DistanceField(dxv.DIST_F32)
        assert np.array_equal(r.view(np.uint32), dr.to_f32(f).view(np.uint32)), key
    finally:
        v.close()


def test_three_frames_in_flight_each_get_their_own_field(dxv, bunny):
    vb, ib, _ = bunny
    v = dxv.Voxelizer(0)
    try:
        v.InitFromArrays(vb, ib)
        plan = [(0, 64, dxv.MODE_REFERENCE, dxv.DIST_SQ_I32), (1, 96, dxv.MODE_PARITY, dxv.DIST_F32), (2, 48, dxv.MODE_REFERENCE_SURFACE, dxv.DIST_SQ_I32)]
        for frame, N, mode, fmt in plan:                                # no synchronisation between any of these
            v.Voxelize(N, mode, sync=False, frameIndex=frame)
            assert v.DistanceField(fmt, sync=False) is True
        v.SyncAll()
        for frame, N, mode, fmt in plan:
            v.SetFrame(frame)
            v.Sync()
            assert v.distance_ms() > 0.0, frame
            assert v.distance_device_ptr()
            want = dr.distance_sq(v.Grid())
            got = v.Distance()
            assert got.shape == (N, N, N)
            assert np.array_equal(got.view(np.uint32), (dr.to_f32(want) if fmt == dxv.DIST_F32 else want).view(np.uint32)), frame
    finally:
        v.close()


def test_distance_refuses_with_a_message_and_launches_nothing(dxv, bunny):
    vb, ib, _ = bunny
    v = dxv.Voxelizer(0)
    lib, ctx = v._lib, v._ctx
    try:
        v.InitFromArrays(vb, ib)
        with pytest.raises(dxv.DxvError, match="no grid yet"):         # before any launch
            v.DistanceField()
        assert lib.dxv_distance_device_ptr(ctx) is None and lib.dxv_distance_bytes(ctx) == 0
        v.Voxelize(64, z0=16, nz=32)
        with pytest.raises(dxv.DxvError, match="not a slab or a share"):
            v.DistanceField()
        v.VoxelizeInterleaved(64, 1, 2, 8)
        with pytest.raises(dxv.DxvError, match="not a slab or a share"):
            v.DistanceField()
        v.Voxelize(64)
        for bad in (-1, 2, 7):
            assert lib.dxv_distance_async(ctx, bad) == 1 and "unknown format" in lib.dxv_last_error(ctx).decode()
            assert lib.dxv_distance(ctx, bad) == 1
        assert lib.dxv_distance_device_ptr(ctx) is None and lib.dxv_distance_bytes(ctx) == 0      # nothing was launched by any of those
        first = v.DistanceField(dxv.DIST_SQ_I32)
        assert lib.dxv_distance_bytes(ctx) == 4 * 64 ** 3 and v.distance_device_ptr()
        buf = np.empty(64 ** 3 + 1, np.int32)
        assert lib.dxv_distance_download(ctx, buf.ctypes.data_as(C.c_void_p), buf.nbytes) == 1
        assert "expected 1048576 bytes" in lib.dxv_last_error(ctx).decode()
        assert lib.dxv_distance_download(ctx, None, 4 * 64 ** 3) == 1
        v.Voxelize(64)                                                 # the frame is launched again: its field is stale
        with pytest.raises(dxv.DxvError, match="stale"):
            v.distance_device_ptr()
        assert lib.dxv_distance_bytes(ctx) == 0
        assert lib.dxv_distance_download(ctx, buf.ctypes.data_as(C.c_void_p), 4 * 64 ** 3) == 1 and "stale" in lib.dxv_last_error(ctx).decode()
        assert np.array_equal(v.DistanceField(dxv.DIST_SQ_I32), first)  # ... and a new one is the same field again
    finally:
        v.close()


def test_trim_gives_back_the_scratch_and_the_next_field_is_the_same(dxv, dragon):
    import torch
    vb, ib, _ = dragon
    v = dxv.Voxelizer(0)
    try:
        v.InitFromArrays(vb, ib)
        v.Voxelize(128)
        first = v.DistanceField(dxv.DIST_F32)
        free0 = torch.cuda.mem_get_info()[0]
        v.trim()
        assert torch.cuda.mem_get_info()[0] - free0 >= 6 * 128 ** 3    # the passes' scratch went back
        assert np.array_equal(v.Distance().view(np.uint32), first.view(np.uint32))                # the field itself stayed
        assert np.array_equal(v.DistanceField(dxv.DIST_F32).view(np.uint32), first.view(np.uint32))
    finally:
        v.close()
