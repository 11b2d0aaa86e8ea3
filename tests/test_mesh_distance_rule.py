"""The mesh distance rule (include/dxv.h: dxv_mesh_distance) on the CPU: the numpy restatement on cases whose field can be
written down, its float32 against its float64 twin on seeded soups, the float64 twin against a region-based closest-point routine
written here, the product's routine (csrc/dxv_mesh_distance.h compiled for the CPU: tests/mesh_distance_host.py) against the
restatement bit for bit -- as a plain loop and through a hierarchy with the kernel's cull rule -- what the header declares, and the
kernels' resources."""
import os
import re
import subprocess

import numpy as np
import pytest

import mesh_distance_host as mh
import mesh_distance_restated as mr
from conftest import ROOT

F32 = np.float32
NO = mr.NO_TRIANGLE


def both(points, tris, index=None, cap=None):
    """(d2, tri) of the restatement, asserted equal to the product's plain loop and to its walk"""
    points = np.asarray(points, F32).reshape(-1, 3)
    tris = np.asarray(tris, F32).reshape(-1, 3, 3)
    d2, tri = mr.nearest(points, tris, index, cap)
    for name, fn in (("loop", mh.brute), ("walk", mh.walk)):
        g2, gtri = fn(points, tris, index, np.inf if cap is None else cap)
        assert np.array_equal(g2.view(np.uint32), d2.view(np.uint32)), name
        assert np.array_equal(gtri, tri), name
    return d2, tri


# ---- cases whose field can be written down (every number a dyadic fraction: float32 is exact) --------------------------------------
TRI = [[0, 0, 0], [1, 0, 0], [0, 1, 0]]                                # in the plane z = 0


def test_single_triangle_interior_edge_vertex():
    points = [[0.25, 0.25, 0.5],        # over the interior: the foot of the perpendicular
              [0.25, 0.25, -0.5],
              [0.25, 0.5, 0.0],         # on it
              [0.5, -0.5, 0.0],         # over the edge a b, in the plane
              [0.5, -0.5, 0.5],         # ... and above it
              [-0.5, -0.5, 0.0],        # over the vertex a
              [-0.75, -1.0, 0.5],
              [2.0, -1.0, 0.0],         # over the vertex b
              [1.0, 1.0, 0.0]]          # over the edge b c: nearest point (0.5, 0.5, 0)
    want = [0.25, 0.25, 0.0, 0.25, 0.5, 0.5, 0.5625 + 1.0 + 0.25, 2.0, 0.5]
    d2, tri = both(points, [TRI])
    assert np.array_equal(d2, np.asarray(want, F32)) and np.all(tri == 0)
    f = mr.value(d2, np.zeros(len(want), np.uint8), mr.UNITS_F32, 16)
    assert np.array_equal(f, np.sqrt(np.asarray(want, F32)))
    g = mr.value(d2, np.ones(len(want), np.uint8), mr.VOXELS_F32, 16)  # negative where the grid's byte is set, voxel units: x N / 2
    assert np.array_equal(g, -(np.sqrt(np.asarray(want, F32)) * F32(8))) and np.signbit(g).all()
    assert np.array_equal(mh.value(d2, np.ones(len(want), np.uint8), mr.VOXELS_F32, 16).view(np.uint32), g.view(np.uint32))


def test_degenerate_triangles_fall_to_the_edge_terms():
    p = [[0.5, 0.25, 0.5], [-1.0, 0.0, 0.0], [2.0, 0.5, 0.0], [0.5, 0.5, 0.0]]
    a = [0.5, 0.25, -0.5]
    d2, _ = both(p, [[a, a, a]])                                        # a point triangle: |p - a|^2
    assert np.array_equal(d2, np.asarray([1.0, 2.25 + 0.0625 + 0.25, 2.25 + 0.0625 + 0.25, 0.0625 + 0.25], F32))
    d2, _ = both(p, [[[0, 0, 0], [0, 0, 0], [1, 0, 0]]])                # a zero-length edge: to the segment (0,0,0) - (1,0,0)
    assert np.array_equal(d2, np.asarray([0.0625 + 0.25, 1.0, 1.0 + 0.25, 0.25], F32))
    d2, _ = both(p, [[[0, 0, 0], [1, 0, 0], [0.5, 0, 0]]])              # collinear vertices
    assert np.array_equal(d2, np.asarray([0.0625 + 0.25, 1.0, 1.0 + 0.25, 0.25], F32))
    for t in ([[a, a, a]], [[[0, 0, 0], [0, 0, 0], [1, 0, 0]]], [[[0, 0, 0], [1, 0, 0], [0.5, 0, 0]]]):
        assert not np.isnan(mr.f_all(np.asarray(p, F32), np.asarray(t, F32))).any()


def test_band_cap_and_no_triangle_beyond_it():
    N, band = 8, 1                                                      # h = 0.25, R = 0.25, cap = 0.0625
    cap = mr.cap_of(N, band)
    assert cap == F32(0.0625) and mh.cap(N, band) == cap and mr.cap_of(N, 0) is None and np.isinf(mh.cap(N, 0))
    points = [[0.25, 0.25, 0.125], [0.25, 0.25, 0.25], [0.25, 0.25, 0.5], [3.0, 3.0, 3.0]]
    d2, tri = both(points, [TRI], index=[7], cap=cap)
    assert np.array_equal(d2, np.asarray([0.015625, 0.0625, 0.0625, 0.0625], F32))
    assert tri.tolist() == [7, 7, NO, NO]                               # f == cap keeps its triangle: only a strictly smaller cap drops it
    for fmt in (mr.VOXELS_F32, mr.UNITS_F32):
        f = mr.value(d2, [0, 1, 0, 1], fmt, N)
        assert abs(f[2]) == (F32(1.0) if fmt == mr.VOXELS_F32 else F32(0.25)) and f[1] < 0 and f[3] < 0 and f[2] > 0


def test_tie_rule_smallest_index_among_equal_f():
    points = np.asarray([[0.25, 0.25, 0.5], [0.5, -0.5, 0.25], [-1, -1, 0], [0.5, 0.5, 1.0]], F32)
    d2, tri = both(points, [TRI, TRI, TRI], index=[9, 4, 6])            # identical triangles
    assert tri.tolist() == [4, 4, 4, 4]
    other = [[1, 0, 0], [0, 0, 0], [0, -1, 0]]                          # shares the edge a b, wound the other way
    for index, want in (([5, 2], 2), ([2, 5], 2), ([0, 0xFFFFFFFE], 0)):
        d2, tri = both([[0.5, 0.0, 0.5], [0.25, 0.0, 0.0], [0.0, 0.0, 1.0]], [TRI, other], index=index)
        assert np.array_equal(d2, np.asarray([0.25, 0.0, 1.0], F32)) and tri.tolist() == [want] * 3
    d2, tri = both([[0.25, 0.5, 0.5], [0.25, -0.5, 0.5]], [TRI, other], index=[5, 2])   # off the shared edge: the nearer one, whatever its index
    assert tri.tolist() == [5, 2]


# ---- accuracy: float32 against the same formula in float64 -----------------------------------------------------------------------
def query_points(seed, n=1500):
    rng = np.random.default_rng(seed)
    return np.concatenate([rng.uniform(-1, 1, (n, 3)), mr.grid_points(8).astype(np.float64)]).astype(F32)


@pytest.mark.parametrize("kind", mr.SOUPS)
def test_float32_is_within_2pow16_of_float64_and_never_undershoots_by_2pow20(kind):
    tris = mr.soup(kind, 400, 11)
    points = query_points(12)
    f32 = mr.f_all(points, tris, F32)
    f64 = mr.f_all(points, tris, np.float64)
    assert f32.dtype == F32 and f64.dtype == np.float64 and np.isfinite(f32).all() and np.isfinite(f64).all()
    err = np.sqrt(f32.astype(np.float64)) - np.sqrt(f64)               # every (point, triangle) pair, not only the minimum
    print(kind, "sqrt(f32) - sqrt(f64): min %.3g max %.3g" % (err.min(), err.max()))
    assert err.max() <= 2.0 ** -16 and err.min() >= -2.0 ** -20
    d32, _ = mr.nearest(points, tris)
    d64, _ = mr.nearest(points, tris, dtype=np.float64)
    err = np.sqrt(d32.astype(np.float64)) - np.sqrt(d64)
    assert err.max() <= 2.0 ** -16 and err.min() >= -2.0 ** -20


def closest_point_by_regions(p, a, b, c):
    """float64 squared distance by the textbook Voronoi-region test (C. Ericson, Real-Time Collision Detection, 5.1.5), one point and
    one triangle per row: nothing shared with the restatement but the inputs"""
    ab, ac, ap = b - a, c - a, p - a
    d1, d2 = (ab * ap).sum(1), (ac * ap).sum(1)
    bp = p - b
    d3, d4 = (ab * bp).sum(1), (ac * bp).sum(1)
    cp = p - c
    d5, d6 = (ab * cp).sum(1), (ac * cp).sum(1)
    vc, vb, va = d1 * d4 - d3 * d2, d5 * d2 - d1 * d6, d3 * d6 - d5 * d4
    with np.errstate(divide="ignore", invalid="ignore"):
        q = a + ab * (vb / (va + vb + vc))[:, None] + ac * (vc / (va + vb + vc))[:, None]          # inside the face
        q = np.where(((va <= 0) & (d4 - d3 >= 0) & (d5 - d6 >= 0))[:, None], b + (c - b) * ((d4 - d3) / ((d4 - d3) + (d5 - d6)))[:, None], q)
        q = np.where(((vb <= 0) & (d2 >= 0) & (d6 <= 0))[:, None], a + ac * (d2 / (d2 - d6))[:, None], q)
        q = np.where(((vc <= 0) & (d1 >= 0) & (d3 <= 0))[:, None], a + ab * (d1 / (d1 - d3))[:, None], q)
    q = np.where(((d6 >= 0) & (d5 <= d6))[:, None], c, q)
    q = np.where(((d3 >= 0) & (d4 <= d3))[:, None], b, q)
    q = np.where(((d1 <= 0) & (d2 <= 0))[:, None], a, q)
    return ((p - q) ** 2).sum(1)


def test_float64_restatement_agrees_with_a_region_based_routine():
    rng = np.random.default_rng(21)
    K = 20000
    a = rng.uniform(-1, 1, (K, 3))
    u, v = rng.normal(size=(K, 3)), rng.normal(size=(K, 3))
    u /= np.linalg.norm(u, axis=1)[:, None]
    v -= u * (u * v).sum(1)[:, None]
    v /= np.linalg.norm(v, axis=1)[:, None]
    s = rng.uniform(0.2, 1.0, (K, 1))
    b = a + s * u                                                        # well shaped: two edges of comparable length, 45 .. 135 degrees apart
    ang = rng.uniform(np.pi / 4, 3 * np.pi / 4, (K, 1))
    c = a + s * rng.uniform(0.7, 1.3, (K, 1)) * (np.cos(ang) * u + np.sin(ang) * v)
    tris = np.stack([a, b, c], 1).astype(F32).astype(np.float64)
    p = rng.uniform(-1.5, 1.5, (K, 3)).astype(F32).astype(np.float64)
    ours = np.array([mr.f_all(p[i:i + 1], tris[i:i + 1], np.float64)[0, 0] for i in range(0, K, 40)])
    ref = closest_point_by_regions(p[::40], tris[::40, 0], tris[::40, 1], tris[::40, 2])
    assert np.abs(np.sqrt(ours) - np.sqrt(ref)).max() <= 1e-12
    # ... and all K pairs at once through the diagonal of chunks
    for s0 in range(0, K, 500):
        f = mr.f_all(p[s0:s0 + 500], tris[s0:s0 + 500], np.float64)
        ref = closest_point_by_regions(p[s0:s0 + 500], tris[s0:s0 + 500, 0], tris[s0:s0 + 500, 1], tris[s0:s0 + 500, 2])
        assert np.abs(np.sqrt(np.diagonal(f)) - np.sqrt(ref)).max() <= 1e-12


# ---- the product's routine, compiled for the CPU ---------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", mr.SOUPS)
def test_product_loop_and_walk_equal_the_restatement_bit_for_bit(kind):
    tris = mr.soup(kind, 500, 31)
    index = np.random.default_rng(32).permutation(len(tris)).astype(np.uint32) + 1000      # the caller's indices are not the positions
    points = query_points(33)
    d2, tri = both(points, tris, index)
    assert (tri != NO).all() and np.isfinite(d2).all()
    cap = mr.cap_of(64, 1)                                             # R = 1 / 32: some points within, some beyond, in every soup
    c2, ctri = both(points, tris, index, cap)
    assert np.array_equal(c2, np.minimum(d2, cap)) and np.array_equal(ctri, np.where(cap < d2, np.uint32(NO), tri))
    assert (ctri == NO).any() and (ctri != NO).any()
    one2, onetri = both(points, tris[:1], index[:1])                    # a tree with no internal node
    assert (onetri == index[0]).all()


def test_a_negative_margin_is_seen_on_the_sliver_soup():
    tris = mr.soup("sliver", 500, 31)
    points = query_points(33)
    d2, tri = mr.nearest(points, tris)
    w2, wtri = mh.walk(points, tris, rel=0.75, ab=-1e-6)                # culls what it must not: the check above would notice
    assert (w2.view(np.uint32) != d2.view(np.uint32)).any() and (w2 >= d2).all()
    rel, ab = mh.margin(tris)
    assert rel == F32(1 + 2.0 ** -9) and ab == F32(2.0 ** -26)          # the root box lies inside [-1, 1]^3: M = 1
    assert mh.margin(tris * F32(3))[1] == F32(2.0 ** -26) * (np.abs(tris * F32(3)).max() * np.abs(tris * F32(3)).max())


# ---- the boundary ----------------------------------------------------------------------------------------------------------------
ENTRIES = {"dxv_mesh_distance_async", "dxv_mesh_distance", "dxv_mesh_distance_device_ptr", "dxv_mesh_distance_bytes",
           "dxv_mesh_distance_download", "dxv_mesh_distance_triangles_device_ptr", "dxv_mesh_distance_triangles_download",
           "dxv_mesh_distance_ms"}


def test_header_declares_the_mesh_distance_entries(tmp_path):
    text = open(os.path.join(ROOT, "include", "dxv.h")).read()
    names = set(re.findall(r"DXV_API\s+[\w\s\*]+?\b(dxv_\w+)\s*\(", text))
    assert ENTRIES <= names
    assert re.search(r"#define DXV_API_VERSION 7\b", text)             # new entries only: no signature or struct changed
    assert re.search(r"\bmdistwalk 0\|1\b", text)                      # the option is in the header's list
    src = tmp_path / "use.c"
    src.write_text('#include "dxv.h"\n'
                   'int main(void) { dxv_ctx* c = 0; float f = 0; uint32_t t = 0;\n'
                   '  int a[DXV_MDIST_VOXELS_F32 == 0 && DXV_MDIST_UNITS_F32 == 1 ? 1 : -1]; (void)a;\n'
                   '  return dxv_mesh_distance_async(c, DXV_MDIST_UNITS_F32, 4u, 1) + dxv_mesh_distance(c, DXV_MDIST_VOXELS_F32, 0u, 0)\n'
                   '       + (dxv_mesh_distance_device_ptr(c) != 0) + (dxv_mesh_distance_triangles_device_ptr(c) != 0)\n'
                   '       + (int)dxv_mesh_distance_bytes(c) + dxv_mesh_distance_download(c, &f, sizeof f)\n'
                   '       + dxv_mesh_distance_triangles_download(c, &t, sizeof t) + dxv_mesh_distance_ms(c, &f); }\n')
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), "-c", str(src),
                           "-o", str(tmp_path / "use.o")])
    from dxrvoxelizer_amd import _lib
    assert _lib.API_VERSION == 7 and ENTRIES <= set(_lib.SYMBOLS)
    import dxrvoxelizer_amd
    assert (dxrvoxelizer_amd.MDIST_VOXELS_F32, dxrvoxelizer_amd.MDIST_UNITS_F32) == (0, 1)
    for method in ("MeshDistanceField", "MeshDistance", "MeshDistanceTriangles", "mesh_distance_device_ptr", "mesh_distance_ms"):
        assert callable(getattr(dxrvoxelizer_amd.Voxelizer, method))


def test_mesh_distance_kernels_use_no_scratch_memory(dxvlib):
    from dxrvoxelizer_amd import build
    if not os.path.exists(os.path.join(build.OBJDIR, "mesh_distance.usage")):
        build.build(force=True)
    res = {k: v for k, v in build.kernel_resources("mesh_distance").items() if "k_mesh_distance" in k}
    assert len(res) == 2, sorted(res)                                  # the walk and the brute-force kernel
    for k, v in res.items():
        assert v["scratch"] == 0, k
