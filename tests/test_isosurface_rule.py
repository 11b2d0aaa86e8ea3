"""The isosurface rule (include/dxv.h: dxv_isosurface) on the CPU: the product's routines (csrc/dxv_isosurface.h compiled
for the CPU and driven in the kernels' order: tests/isosurface_host.py) against the numpy restatement (tests/isosurface_restated.py) byte
for byte, the counts of grids that can be counted by hand, closedness and orientation of every mesh, what the header declares, and the
kernels' resources."""
import os
import re
import subprocess

import numpy as np
import pytest

import distance_restated as dr
import isosurface_host as ih
import isosurface_restated as ir
from conftest import ROOT

F32 = np.float32
BOUND = np.asarray([0.125, -0.75, 2.5, 1.75], F32)


def grid_field(grid):
    """DXV_DIST_F32 of a grid by the min-plus restatement (every voxel against every voxel of its row, column and pile)"""
    return dr.distance_f32(np.asarray(grid, np.uint8))


def random_grid(N, seed):
    return (np.random.default_rng(seed).random((N, N, N)) < 0.5).astype(np.uint8)


def checkerboard(N):
    z, y, x = np.indices((N, N, N))
    return ((x + y + z) & 1).astype(np.uint8)


def one_voxel(N):
    g = np.zeros((N, N, N), np.uint8)
    g[N // 2, N // 2, N // 2] = 1
    return g


def box(N, w):
    g = np.zeros((N, N, N), np.uint8)
    lo = (N - w) // 2
    g[lo:lo + w, lo:lo + w, lo:lo + w] = 1
    return g


def sphere_field(N, units):
    """distance to a sphere of radius 0.6 (normalised) about a point off the lattice, at the voxel centres, in voxels or normalised units"""
    c = ((np.arange(N, dtype=np.float64) + 0.5) / N * 2 - 1)
    z, y, x = np.meshgrid(c, c, c, indexing="ij")
    d = np.sqrt((x - 0.07) ** 2 + (y + 0.03) ** 2 + (z - 0.11) ** 2) - 0.6
    return (d if units else d * (N / 2)).astype(F32)


def planted_field():
    """a sphere with exact zeros of both signs, NaNs and infinities planted where its surface runs"""
    f = sphere_field(12, False)
    near = np.argwhere(np.abs(f) < 0.6)
    rng = np.random.default_rng(5)
    for n, (k, j, i) in enumerate(near[rng.permutation(len(near))[:60]]):
        f[k, j, i] = (F32(0.0), F32(-0.0), F32(np.nan), F32(np.inf), F32(-np.inf))[n % 5]
    return f


def cases():
    """(name, field, iso, P)"""
    for N in (4, 8, 11):
        yield f"random {N}", grid_field(random_grid(N, N)), 0.0, 1.0
    yield "checkerboard 6", grid_field(checkerboard(6)), 0.0, 1.0
    yield "all solid 4", grid_field(np.ones((4, 4, 4), np.uint8)), 0.0, 1.0           # -INF everywhere: the crossings at one half
    yield "all empty 4", grid_field(np.zeros((4, 4, 4), np.uint8)), 0.0, 1.0
    yield "one voxel 5", grid_field(one_voxel(5)), 0.0, 1.0
    yield "box 5 in 11", grid_field(box(11, 5)), 0.0, 1.0
    for units in (False, True):
        P = ir.voxel(12, units)
        for k in (0.0, 0.5, -0.5):
            yield f"sphere 12 {'units' if units else 'voxels'} iso {k} P", sphere_field(12, units), F32(k) * P, P
    yield "planted 12", planted_field(), 0.0, 1.0
    yield "planted 12 iso 0.25", planted_field(), 0.25, 1.0
    yield "slab 65", grid_field(slab65()), 0.0, 1.0                    # a cell row of 66 cells: two words, the surface runs through the boundary


def slab65():
    g = np.zeros((65, 65, 65), np.uint8)
    g[30:34, 20:24, 2:65] = 1                                           # along x from voxel 2 to the grid's border: cells 63, 64 and 65 carry it on
    return g


CASES = list(cases())


@pytest.fixture(scope="module")
def meshes():
    """the restatement of every case in both spaces, made once"""
    return {(name, space): ir.extract(f, iso, P, space, BOUND) for name, f, iso, P in CASES for space in (ir.SPACE_VOXELS, ir.SPACE_OBJECT)}


@pytest.mark.parametrize("space", [ir.SPACE_VOXELS, ir.SPACE_OBJECT])
@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_product_routine_equals_the_restatement_byte_for_byte(meshes, case, space):
    name, f, iso, P = case
    vb, ib = meshes[name, space]
    hv, hi = ih.extract(f, iso, P, space, BOUND)
    assert hv.shape == vb.shape and hi.shape == ib.shape, (hv.shape, vb.shape, hi.shape, ib.shape)
    assert np.array_equal(hv.view(np.uint32), vb.view(np.uint32))
    assert hi.dtype == np.uint32 and np.array_equal(hi, ib)


@pytest.mark.parametrize("space", [ir.SPACE_VOXELS, ir.SPACE_OBJECT])
@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_every_mesh_is_closed_and_points_outwards(meshes, case, space):
    vb, ib = meshes[case[0], space]
    assert len(ib) % 6 == 0 and (len(ib) == 0) == (len(vb) == 0)
    if len(ib):
        assert ib.max() < len(vb) and len(np.unique(ib)) == len(vb)    # every vertex is used
    assert ir.directed_edges_pair_up(ib)
    if len(ib):
        assert ir.signed_volume(vb, ib) > 0.0


@pytest.mark.parametrize("name,vertices,triangles,volume", [("all solid 4", 98, 192, 53.875), ("box 5 in 11", 152, 300, 111.875),
                                                            ("one voxel 5", 8, 12, None), ("all empty 4", 0, 0, None)])
def test_counts_of_grids_that_can_be_counted_by_hand(meshes, name, vertices, triangles, volume):
    vb, ib = meshes[name, ir.SPACE_VOXELS]
    assert (len(vb), len(ib) // 3) == (vertices, triangles)
    if volume is not None:
        assert abs(ir.signed_volume(vb, ib) - volume) < 1e-4


def test_volume_of_a_box_lies_between_its_centres_and_its_voxels():
    # the surface sits half a voxel outside the outermost centres and the nets only cut corners: (w - 1)^3 <= volume <= w^3
    for N, w in ((11, 5), (12, 4), (14, 7)):
        vb, ib = ir.extract(grid_field(box(N, w)))
        vol = ir.signed_volume(vb, ib)
        print(N, w, vol)
        assert (w - 1) ** 3 <= vol <= w ** 3


def test_normals_point_out_of_a_sphere_and_vertices_lie_on_it():
    N = 12
    vb, ib = ir.extract(sphere_field(N, False))
    centre = (np.asarray([0.07, -0.03, 0.11]) + 1) * N / 2 - 0.5        # in voxel index space
    r = vb[:, :3].astype(np.float64) - centre
    dist = np.linalg.norm(r, axis=1)
    assert np.abs(dist - 0.6 * N / 2).max() < 0.5                      # within half a voxel of the sphere
    assert ((r / dist[:, None]) * vb[:, 3:]).sum(1).min() > 0.9
    assert np.abs(np.linalg.norm(vb[:, 3:].astype(np.float64), axis=1) - 1).max() < 1e-6


def test_object_space_is_the_voxel_centres_of_the_ray_rules():
    f = sphere_field(12, False)
    v, iv = ir.extract(f)
    o, io = ir.extract(f, space=ir.SPACE_OBJECT, bound=BOUND)
    q = (v[:, :3].astype(np.float64) + 0.5) / 12 * 2 - 1
    q[:, 1] = -q[:, 1]
    assert np.abs(o[:, :3] - (q * BOUND[3] + BOUND[:3])).max() < 1e-5
    assert np.array_equal(o[:, [3, 5]], v[:, [3, 5]]) and np.array_equal(o[:, 4], -v[:, 4])
    assert np.array_equal(io.reshape(-1, 3), iv.reshape(-1, 3)[:, ::-1])


# ---- the boundary ----------------------------------------------------------------------------------------------------------------
ENTRIES = {"dxv_isosurface_async", "dxv_isosurface", "dxv_isosurface_counts", "dxv_isosurface_vertices_device_ptr",
           "dxv_isosurface_indices_device_ptr", "dxv_isosurface_vertices_download", "dxv_isosurface_indices_download", "dxv_isosurface_ms"}


def test_header_declares_the_isosurface_entries(tmp_path):
    text = open(os.path.join(ROOT, "include", "dxv.h")).read()
    names = set(re.findall(r"DXV_API\s+[\w\s\*]+?\b(dxv_\w+)\s*\(", text))
    assert ENTRIES <= names
    assert re.search(r"#define DXV_API_VERSION 7\b", text)             # new entries only: no signature or struct changed
    src = tmp_path / "use.c"
    src.write_text('#include "dxv.h"\n'
                   'int main(void) { dxv_ctx* c = 0; float f = 0; uint32_t v = 0, t = 0;\n'
                   '  int a[DXV_ISO_MESH_DISTANCE == 0 && DXV_ISO_GRID_DISTANCE == 1 && DXV_ISO_SPACE_VOXELS == 0 && DXV_ISO_SPACE_OBJECT == 1 ? 1 : -1]; (void)a;\n'
                   '  return dxv_isosurface_async(c, DXV_ISO_GRID_DISTANCE, 0.5f, DXV_ISO_SPACE_VOXELS) + dxv_isosurface(c, DXV_ISO_MESH_DISTANCE, 0.0f, DXV_ISO_SPACE_OBJECT)\n'
                   '       + dxv_isosurface_counts(c, &v, &t) + (dxv_isosurface_vertices_device_ptr(c) != 0) + (dxv_isosurface_indices_device_ptr(c) != 0)\n'
                   '       + dxv_isosurface_vertices_download(c, &f, sizeof f) + dxv_isosurface_indices_download(c, &t, sizeof t) + dxv_isosurface_ms(c, &f); }\n')
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), "-c", str(src),
                           "-o", str(tmp_path / "use.o")])
    from dxrvoxelizer_amd import _lib
    assert _lib.API_VERSION == 7 and ENTRIES <= set(_lib.SYMBOLS)
    import dxrvoxelizer_amd
    assert (dxrvoxelizer_amd.ISO_MESH_DISTANCE, dxrvoxelizer_amd.ISO_GRID_DISTANCE) == (0, 1)
    assert (dxrvoxelizer_amd.ISO_SPACE_VOXELS, dxrvoxelizer_amd.ISO_SPACE_OBJECT) == (0, 1)
    for method in ("Isosurface", "IsosurfaceCounts", "IsosurfaceMesh", "isosurface_device_ptrs", "isosurface_ms"):
        assert callable(getattr(dxrvoxelizer_amd.Voxelizer, method))
    mirror = open(os.path.join(ROOT, "include", "dxv_voxelizer.hpp")).read()
    assert "dxv_isosurface_async" in mirror and "DownloadIsosurface" in mirror


def test_isosurface_kernels_use_no_scratch_memory(dxvlib):
    from dxrvoxelizer_amd import build
    if not os.path.exists(os.path.join(build.OBJDIR, "isosurface.usage")):
        build.build(force=True)
    res = {k: v for k, v in build.kernel_resources("isosurface").items() if "k_iso" in k}
    assert len(res) == 2, sorted(res)                                  # count, emit (the scan between them is csrc/scan.hip's: tests/test_scan_resources.py)
    for k, v in res.items():
        assert v["scratch"] == 0, k
        assert v["lds"] == 0, k
