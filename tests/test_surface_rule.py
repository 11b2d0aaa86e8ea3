"""The surface rule (DXV_MODE_SURFACE) on the CPU: the restatement's own cases (faces, edges and corners touched, one
float32 ulp beyond a face, degenerate triangles, the column walk of a large triangle, float32 == float64 on the shipped assets), and
the boundary that declares the two new modes.  No GPU needed."""
import json
import os
import re

import numpy as np
import pytest

from conftest import GOLD, ROOT
import surface_restated as sr

F = np.float32


def grid_of(tris, N):
    return sr.surface_grid(np.asarray(tris, F).reshape(-1, 3, 3), N)


def face(N, i):
    """The x = const plane between voxels i - 1 and i (exact for a power-of-two N)."""
    return F(sr.centres(N, i)) - F(1) / F(N)


# ---- the restatement ------------------------------------------------------------------------------------------------
def test_triangle_on_a_voxel_face_marks_both_neighbours():
    N = 16
    x = face(N, 8)
    assert x == F(0.0)
    # a small triangle in the plane x = 0, inside the y/z extent of voxel row (iy, iz) = (7, 8) only
    c_y, c_z = -sr.centres(N, 7), sr.centres(N, 8)
    d = F(0.01)
    g = grid_of([[x, c_y - d, c_z - d], [x, c_y + d, c_z - d], [x, c_y, c_z + d]], N)
    assert sorted(zip(*np.nonzero(g))) == [(8, 7, 7), (8, 7, 8)]


@pytest.mark.parametrize("N", [16, 64])
def test_one_ulp_beyond_a_face_leaves_the_near_voxel(N):
    i = N // 2 + 3
    x = face(N, i)
    c_y, c_z = -sr.centres(N, 5), sr.centres(N, 6)
    d = F(0.1) / F(N)
    tri = lambda x: [[x, c_y - d, c_z - d], [x, c_y + d, c_z - d], [x, c_y, c_z + d]]
    on = grid_of(tri(x), N)
    assert set(np.nonzero(on)[2]) == {i - 1, i}
    beyond = grid_of(tri(np.nextafter(x, F(2))), N)
    assert set(np.nonzero(beyond)[2]) == {i}
    below = grid_of(tri(np.nextafter(x, F(-2))), N)
    assert set(np.nonzero(below)[2]) == {i - 1}


def test_touching_only_a_corner_or_an_edge_marks_the_voxel():
    N = 16
    x0, y0, z0 = face(N, 4), -face(N, 4), face(N, 4)        # the corner shared by voxels (3..4, 3..4, 3..4); y = -x0 is a face too
    h = F(1) / F(N)
    # a triangle in the plane x + y' + z = const through that corner, reaching away from it: touches the eight voxels around the
    # corner only at the corner or along their edges
    g = grid_of([[x0, y0, z0], [x0 - h, y0, z0], [x0, y0, z0 - h]], N)
    assert g[3, 3, 3] and g[4, 4, 4] and g[4, 3, 4]
    # a lone point exactly on the corner (a degenerate triangle) marks all eight voxels around it
    p = grid_of([[x0, y0, z0]] * 3, N)
    assert int(p.sum()) == 8 and p[3:5, 3:5, 3:5].all()
    # a segment along the edge x = x0, z = z0 in y marks the four voxels around that edge in each row it crosses
    s = grid_of([[x0, -sr.centres(N, 6), z0], [x0, -sr.centres(N, 9), z0], [x0, -sr.centres(N, 9), z0]], N)
    assert int(s.sum()) == 4 * 4 and s[3:5, 6:10, 3:5].all()


def test_degenerate_triangles_are_decided_by_the_other_tests():
    N = 16
    c = sr.centres(N, np.arange(N))
    # a point inside voxel (x 2, y 3, z 5) and a segment inside one row
    pt = grid_of([[c[2], -c[3], c[5]]] * 3, N)
    assert sorted(zip(*np.nonzero(pt))) == [(5, 3, 2)]
    seg = grid_of([[c[2], -c[3], c[5]], [c[9], -c[3], c[5]], [c[9], -c[3], c[5]]], N)
    assert sorted(zip(*np.nonzero(seg))) == [(5, 3, x) for x in range(2, 10)]
    # every candidate agrees with the voxel-by-voxel application
    tris = np.asarray([[[c[2], -c[3], c[5]]] * 3, [[c[2], -c[3], c[5]], [c[9], -c[7], c[1]], [c[9], -c[7], c[1]]]], F)
    assert np.array_equal(sr.surface_grid(tris, N), sr.brute_grid(tris, N))


def test_large_tilted_triangle_column_walk_equals_the_rule_everywhere():
    N = 16
    tris = np.asarray([[[-0.93, 0.71, -0.4], [0.88, -0.95, 0.2], [0.1, 0.9, 0.97]],
                       [[-1.0, -1.0, -1.0], [1.0, 1.0, -1.0], [1.0, -1.0, 1.0]]], F)
    walked = sr.surface_grid(tris, N, large=1)              # every triangle through the column walk
    assert walked.sum() > 300
    assert np.array_equal(walked, sr.brute_grid(tris, N))
    assert np.array_equal(sr.surface_grid(tris, N), walked)


@pytest.mark.parametrize("name,count", [("turingbowl", 15775), ("bunny", 14175), ("dragon", 10231)])
def test_float32_equals_float64_on_the_assets_at_64(name, count):
    d = np.load(os.path.join(GOLD, "meshes", name + ".npz"))
    tris = sr.normalised_tris(d["vb"], d["ib"])
    g32 = sr.surface_grid(tris, 64)
    assert int(g32.sum()) == count
    assert np.array_equal(g32, sr.surface_grid(tris, 64, np.float64))


def test_normalisation_is_the_scene_rule(orc):
    d = np.load(os.path.join(GOLD, "meshes", "bunny.npz"))
    c, w = sr.bound_of(d["vb"])
    _, b = orc.bound(d["vb"])
    assert np.array_equal(np.r_[c, w].astype(F), b)
    sc = orc.Scene(d["vb"], d["ib"])
    tris = sr.normalised_tris(d["vb"], d["ib"])
    for k in (0, 1, 777, len(tris) - 1):
        p, _ = sc.tri(k)
        assert np.array_equal(p, tris[k])


def test_fixture_file_is_consistent():
    with open(os.path.join(GOLD, "surface.json")) as fh:
        fx = json.load(fh)
    assert set(fx) == {"torus1m/512", "dragon9/512", "cube/1024", "tetrahedron/1024"}
    for key, e in fx.items():
        assert e["reference_surface"]["count"] >= max(e["surface"]["count"], e["solid"]["count"]), key
        assert e["f32_f64_differences"] == 0, key
    # the cube's faces lie on the grid's outer voxel faces: its surface is the outermost layer, 6 N^2 - 12 N + 8 voxels
    assert fx["cube/1024"]["surface"]["count"] == 6 * 1024 ** 2 - 12 * 1024 + 8


# ---- the boundary -----------------------------------------------------------------------------------------------------
def test_header_declares_the_surface_modes():
    with open(os.path.join(ROOT, "include", "dxv.h")) as fh:
        h = fh.read()
    assert re.search(r"DXV_MODE_SURFACE\s*=\s*2\b", h)
    assert re.search(r"DXV_MODE_REFERENCE_SURFACE\s*=\s*3\b", h)
    assert re.search(r"#define DXV_API_VERSION 7\b", h)
    for hpp in ("dxv_voxelizer.hpp", "dxv_multi.hpp"):
        with open(os.path.join(ROOT, "include", hpp)) as fh:
            src = fh.read()
        assert "SURFACE = DXV_MODE_SURFACE" in src and "REFERENCE_SURFACE = DXV_MODE_REFERENCE_SURFACE" in src, hpp


def test_package_exports_the_surface_modes(dxvlib):
    import dxrvoxelizer_amd as dxv
    assert (dxv.MODE_REFERENCE, dxv.MODE_PARITY, dxv.MODE_SURFACE, dxv.MODE_REFERENCE_SURFACE) == (0, 1, 2, 3)
    assert dxvlib.dxv_api_version() == 7


def test_surface_kernels_use_no_scratch(dxvlib):
    from dxrvoxelizer_amd import build
    res = build.kernel_resources("surface")
    kernels = {k: v for k, v in res.items() if "k_surface_tris" in k or "k_surface_large" in k}
    assert len(kernels) == 2, sorted(res)
    for k, v in kernels.items():
        assert v["scratch"] == 0, (k, v)
        assert v["vgprs"] <= 128, (k, v)


# ---- the kernel's candidate box (csrc/dxv_surface.h: surface_box, 1/16 voxel of margin; restated as surface_restated.kernel_box) -------
def near_face_triangles(rng, N, count):
    """triangles whose extreme coordinates sit on voxel faces or a float32 ulp either side of them, some with a vertex far outside
    the grid (a refitted mesh may leave its build's bound), some entirely outside"""
    faces = (sr.centres(N, np.arange(N)) - F(1) / F(N)).astype(F)
    faces = np.append(faces, F(1))
    out = []
    for i in range(count):
        t = rng.uniform(-1.1, 1.1, (3, 3)).astype(F)
        t = t[0] + (t - t[0]) * F(rng.choice([0.01, 0.05, 0.3]))             # small to mid-sized
        for k in range(3):                                                    # move the triangle so an extreme sits on a face
            f = faces[rng.integers(len(faces))]
            f = [np.nextafter(f, F(-2)), f, np.nextafter(f, F(2))][rng.integers(3)]
            j = int(np.argmin(t[:, k])) if rng.random() < 0.5 else int(np.argmax(t[:, k]))
            t[:, k] = (t[:, k] + (f - t[j, k])).astype(F)
            t[j, k] = f
        if i % 3 == 1:                                                        # one vertex far away
            t[rng.integers(3)] = (rng.choice([-1, 1], 3) * 10.0 ** rng.uniform(1, 6, 3)).astype(F)
        if i % 7 == 2:                                                        # the whole triangle just outside one side
            k = rng.integers(3)
            t[:, k] = (np.abs(t[:, k] - t[:, k].min()) + np.nextafter(F(1), F(2)) * F(rng.choice([-1, 1]))).astype(F)
            if t[0, k] < 0:
                t[:, k] = -np.abs(t[:, k])
        out.append(t)
    return out


@pytest.mark.parametrize("N", [16, 64])
def test_kernel_candidate_box_holds_every_accepted_voxel(N):
    rng = np.random.default_rng(1234 + N)
    seen = 0
    for t in near_face_triangles(rng, N, 240):
        got = np.argwhere(sr.surface_grid(t[None], N))                       # (z, y, x) of the voxels the test accepts
        box = sr.kernel_box(t, N)
        if box is None:
            assert len(got) == 0, t
            continue
        lo, hi = box
        for axis, col in ((0, 2), (1, 1), (2, 0)):
            assert (got[:, col] >= lo[axis]).all() and (got[:, col] <= hi[axis]).all(), (t, axis, lo, hi)
        seen += len(got)
    assert seen > 1000
