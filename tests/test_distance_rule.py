"""The distance field of a grid (include/dxv.h: dxv_distance) on the CPU: the numpy restatement's own cases (one voxel, two
opposite corners, a plane, empty, full), the product's scans (csrc/dxv_distance.h compiled for the CPU: tests/distance_host.py) against
that restatement on random grids, what the header declares, and the kernels' resources."""
import os
import re
import subprocess

import numpy as np
import pytest

import distance_host
import distance_restated as dr
import grid_sides as gs
from conftest import ROOT


# ---- the restatement against grids whose field can be written down ------------------------------------------------------------
def test_restatement_single_voxel():
    N = 12
    g = np.zeros((N, N, N), np.uint8)
    g[3, 7, 5] = 200                                                   # (any non-zero byte is solid)
    z, y, x = np.indices(g.shape)
    want = (z - 3) ** 2 + (y - 7) ** 2 + (x - 5) ** 2
    want[3, 7, 5] = -1                                                 # the one solid voxel: its nearest empty neighbour, negative
    assert np.array_equal(dr.distance_sq(g), want.astype(np.int32))
    f = dr.distance_f32(g)
    assert f.dtype == np.float32 and f[3, 7, 5] == -1.0 and f[3, 7, 6] == 1.0 and f[0, 0, 0] == np.float32(np.sqrt(np.float32(9 + 49 + 25)))


def test_restatement_two_opposite_corners():
    N = 10
    g = np.zeros((N, N, N), np.uint8)
    g[0, 0, 0] = g[-1, -1, -1] = 1
    d = dr.distance_sq(g)
    z, y, x = np.indices(g.shape)
    near = np.minimum(z * z + y * y + x * x, (N - 1 - z) ** 2 + (N - 1 - y) ** 2 + (N - 1 - x) ** 2)
    near[0, 0, 0] = near[-1, -1, -1] = -1
    assert np.array_equal(d, near.astype(np.int32))
    # a solid grid with two empty corners: the far corner of either sees the other across the whole diagonal only if it must
    h = np.ones((N, N, N), np.uint8)
    h[0, 0, 0] = 0
    assert dr.distance_sq(h)[-1, -1, -1] == -3 * (N - 1) ** 2          # d2 = 3 (N - 1)^2, negative inside


def test_restatement_plane_empty_full():
    N = 8
    g = np.zeros((N, N, N), np.uint8)
    g[:, 3, :] = 1                                                     # the plane y = 3
    y = np.indices(g.shape)[1]
    want = (y - 3) ** 2
    want[:, 3, :] = -1
    assert np.array_equal(dr.distance_sq(g), want.astype(np.int32))
    empty, full = np.zeros((N, N, N), np.uint8), np.full((N, N, N), 255, np.uint8)
    assert np.all(dr.distance_sq(empty) == 0x7fffffff) and np.all(dr.distance_sq(full) == -0x7fffffff)
    assert np.all(dr.distance_f32(empty) == np.inf) and np.all(dr.distance_f32(full) == -np.inf)


def test_restatement_equals_scipy_where_present():
    ndimage = pytest.importorskip("scipy.ndimage")
    rng = np.random.default_rng(5)
    for N, density in ((32, 0.5), (32, 0.02), (48, 0.001)):
        g = (rng.random((N, N, N)) < density).astype(np.uint8)
        if not g.any():
            g[1, 2, 3] = 1
        s = g != 0
        want = np.where(s, -np.rint(ndimage.distance_transform_edt(s) ** 2), np.rint(ndimage.distance_transform_edt(~s) ** 2))
        assert np.array_equal(dr.distance_sq(g), want.astype(np.int32))


# ---- the product's scans, compiled for the CPU, against the restatement -----------------------------------------------------------
@pytest.mark.parametrize("N,density,seed", [(16, 0.5, 1), (16, 0.03, 2), (24, 0.9, 3), (30, 0.5, 4), (32, 0.002, 5), (48, 0.2, 6), (64, 0.5, 7),
                                            (64, 0.01, 8), (64, 0.0003, 9), (64, 0.999, 10)])
def test_product_scans_equal_restatement_on_random_grids(N, density, seed):
    rng = np.random.default_rng(seed)
    g = ((rng.random((N, N, N)) < density) * rng.integers(1, 256, (N, N, N))).astype(np.uint8)
    want = dr.distance_sq(g)
    assert np.array_equal(distance_host.distance(g, 0), want)
    assert np.array_equal(distance_host.distance(g, 1).view(np.uint32), dr.to_f32(want).view(np.uint32))


@pytest.mark.parametrize("N", gs.SWEEP)                                # every even side to 72 (tests/grid_sides.py): every length of a row's last word
def test_product_scans_equal_restatement_on_the_sweep_grids(N):
    for name, g in gs.grids(N):
        want = dr.distance_sq(g)
        assert np.array_equal(distance_host.distance(g, 0), want), (N, name)
        assert np.array_equal(distance_host.distance(g, 1).view(np.uint32), dr.to_f32(want).view(np.uint32)), (N, name)


def test_product_scans_on_shapes_and_sentinels():
    N = 40
    z, y, x = np.indices((N, N, N))
    r2 = (x - 18) ** 2 + (y - 21) ** 2 + (z - 17) ** 2
    shapes = {"ball": r2 < 150, "shell": (r2 < 300) & (r2 >= 120), "slab": (y > 10) & (y < 14), "checker": (x + y + z) % 2 == 0,
              "rods": (x % 7 == 0) & (y % 5 == 0), "empty": r2 < 0, "full": r2 >= 0, "one": r2 == 0}
    for name, s in shapes.items():
        g = s.astype(np.uint8)
        want = dr.distance_sq(g)
        assert np.array_equal(distance_host.distance(g, 0), want), name
        assert np.array_equal(distance_host.distance(g, 1).view(np.uint32), dr.to_f32(want).view(np.uint32)), name
    for N in (2, 4, 66, 130):                                           # the smallest grid; rows of one, two (partial) and three words
        g = np.zeros((N, N, N), np.uint8)
        g[N - 1, 0, N - 1] = 1
        z, y, x = np.indices(g.shape)
        want = ((z - N + 1) ** 2 + y ** 2 + (x - N + 1) ** 2).astype(np.int32)
        want[N - 1, 0, N - 1] = -1
        assert np.array_equal(distance_host.distance(g, 0), want), N


# ---- the boundary ----------------------------------------------------------------------------------------------------------------------
def test_header_declares_the_distance_entries(tmp_path):
    text = open(os.path.join(ROOT, "include", "dxv.h")).read()
    names = set(re.findall(r"DXV_API\s+[\w\s\*]+?\b(dxv_\w+)\s*\(", text))
    assert {"dxv_distance_async", "dxv_distance", "dxv_distance_device_ptr", "dxv_distance_bytes", "dxv_distance_download",
            "dxv_distance_ms"} <= names
    assert re.search(r"#define DXV_API_VERSION 7\b", text)             # new entries only: no signature or struct changed
    src = tmp_path / "use.c"
    src.write_text('#include "dxv.h"\n'
                   'int main(void) { dxv_ctx* c = 0; float ms = 0; int a[DXV_DIST_SQ_I32 == 0 && DXV_DIST_F32 == 1 ? 1 : -1]; (void)a;\n'
                   '  return dxv_distance_async(c, DXV_DIST_F32) + dxv_distance(c, DXV_DIST_SQ_I32) + (dxv_distance_device_ptr(c) != 0)\n'
                   '       + (int)dxv_distance_bytes(c) + dxv_distance_download(c, &ms, sizeof ms) + dxv_distance_ms(c, &ms); }\n')
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), "-c", str(src),
                           "-o", str(tmp_path / "use.o")])
    from dxrvoxelizer_amd import _lib
    assert _lib.API_VERSION == 7 and {"dxv_distance_async", "dxv_distance_ms"} <= set(_lib.SYMBOLS)


def test_distance_kernels_use_no_scratch_memory(dxvlib):
    from dxrvoxelizer_amd import build
    if not os.path.exists(os.path.join(build.OBJDIR, "distance.usage")):
        build.build(force=True)
    res = {k: v for k, v in build.kernel_resources("distance").items() if "k_dist" in k}
    assert len(res) == 4, sorted(res)                                  # rows; columns: 16-bit -> squares, squares -> int32, squares -> float32
    for k, v in res.items():
        assert v["scratch"] == 0, k
        assert v["occupancy"] == 8, k                                  # (a scan is a chain of dependent loads: waves are what hides them)
    assert all(v["lds"] == 0 for k, v in res.items() if "k_dist_columns" in k)      # the stacks live in the output column, not in LDS
