"""The geodesic distance on the GPU (include/dxv.h: dxv_geodesic*): the device's map (uint32 per voxel) and tally equal, as bytes, what the rule
gives for the grid -- by Dijkstra (tests/geodesic_restated.py, form (b)) and by the host library (tests/geodesic_host.py: the product's routines
run serially, held to both restatements by tests/test_geodesic_rule.py) -- on the smallest shapes that still reach each mechanism: a serpentine
whose one path crosses tile faces many times, under three batch sizes; the checkerboard; the limit; a mask in device memory; the details of a
seed list; bytes other than 1; two frames in flight; the same call three times; the flood fill's set; the path on the bunny; the skeleton-length
recipe; what makes the map stale; what the call refuses; dxv_trim; and the C++ mirror."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import geodesic_host as gh
import geodesic_restated as gr
from raycast_restated import write_grid

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TALLY = ("seeds_used", "reached", "unreached", "farthest", "farthest_voxel")
U, X = gr.UNREACHED, gr.NONE


@pytest.fixture(scope="module")
def dxv(dxvlib):
    import dxrvoxelizer_amd
    return dxrvoxelizer_amd


@pytest.fixture(scope="module")
def writer(dxv, bunny):
    """the one Voxelizer, on the bunny, whose frame the grids of this file are written into"""
    vb, ib, _ = bunny
    v = dxv.Voxelizer(0)
    v.InitFromArrays(vb, ib)
    yield v
    v.close()


def check(v, want, of, metric, seeds, limit=0, what=""):
    """Geodesic of the selected frame: map and tally against `want`; returns the map and the info"""
    got = v.Geodesic(of, metric, seeds, limit)
    assert got.dtype == np.uint32 and got.shape == want.shape and got.tobytes() == want.tobytes(), (what, of, metric, limit, int(np.count_nonzero(got != want)))
    info = v.GeodesicInfo()
    assert {k: info[k] for k in TALLY} == gr.tally(want), (what, of, metric, limit)
    return got, info


# ---- rounds and batches ----------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def serpentine():
    g = gr.serpentine(24, 1, 1)                                         # twelve slabs of three tiles each: the one path crosses 35 tile faces
    seeds = gr.smallest_member(g, gr.SOLID)
    return g, seeds, {m: gr.geodesic_dijkstra(g, gr.SOLID, m, seeds) for m in (gr.FACES, gr.CHAMFER)}


@pytest.mark.parametrize("metric", [gr.FACES, gr.CHAMFER])
def test_a_serpentine_under_three_batch_sizes(writer, serpentine, metric):
    g, seeds, want = serpentine
    v = writer
    v.Voxelize(24)
    write_grid(v, g)
    try:
        maps = []
        for batch in (1, 2, 0):
            v.set_option("georounds", batch)
            got, info = check(v, want[metric], gr.SOLID, metric, seeds, what=f"georounds {batch}")
            maps.append(got.tobytes())
            # a word crosses into the next tile only in a round in which that tile runs, and a tile runs only when the round before changed
            # a voxel on its border: the front gains two tiles per round at the most, 35 faces take 18 rounds or more
            assert info["rounds"] > (batch or 16), (batch, info)
            assert info["ms"] > 0.0
        assert maps[0] == maps[1] == maps[2]
        with pytest.raises(dxv_error(), match="georounds"):
            v.set_option("georounds", 65)
    finally:
        v.set_option("georounds", 0)


def dxv_error():
    import dxrvoxelizer_amd
    return dxrvoxelizer_amd.DxvError


@pytest.mark.parametrize("metric", [gr.FACES, gr.CHAMFER])
def test_the_checkerboard(writer, metric):
    g = gr.checkerboard(10)
    v = writer
    v.Voxelize(10)
    write_grid(v, g)
    seed = np.array([0], np.uint32)
    got, info = check(v, gr.geodesic_dijkstra(g, gr.SOLID, metric, seed), gr.SOLID, metric, seed, what="checkerboard")
    if metric == gr.FACES:
        assert (info["reached"], info["unreached"], info["farthest"], info["farthest_voxel"]) == (1, 499, 0, 0)
    else:
        assert (info["reached"], info["unreached"], info["farthest"]) == (500, 0, 52)


@pytest.mark.parametrize("metric", [gr.FACES, gr.CHAMFER])
def test_the_limit(writer, serpentine, metric):
    g, seeds, want = serpentine
    v = writer
    v.Voxelize(24)
    write_grid(v, g)
    out0, info0 = check(v, want[metric], gr.SOLID, metric, seeds, what="no limit")
    occurring = int(np.unique(out0[out0 < U])[40])
    assert (out0 == occurring).any()
    for limit in (3, occurring, info0["farthest"] // 2):
        out, info = check(v, gr.limited(want[metric], limit), gr.SOLID, metric, seeds, limit, "limit")
        members = out0 != X
        assert np.array_equal(out[members], np.where(out0[members] <= limit, out0[members], U)), limit
        assert info["rounds"] <= info0["rounds"] and info["farthest"] <= limit, (limit, info, info0)
    assert (v.Geodesic(gr.SOLID, metric, seeds, occurring) == occurring).any()      # a voxel with G == limit is kept


# ---- seeds ----------------------------------------------------------------------------------------------------------------------------------
def random_grid():
    import grid_sides as gs
    return dict(gs.grids(18))["random 0.3"]


def test_a_mask_seeded_from_a_device_tensor(writer):
    import torch
    g = random_grid()
    v = writer
    v.Voxelize(18)
    write_grid(v, g)
    rng = np.random.default_rng(11)
    mask = (rng.random(g.shape) < 0.01).astype(np.uint8) * 0x80
    t = torch.from_numpy(mask).cuda()
    for of in (gr.SOLID, gr.EMPTY):
        want = gr.geodesic_dijkstra(g, of, gr.CHAMFER, mask)
        got, info = check(v, want, of, gr.CHAMFER, t, what="device mask")
        assert info["seeds_used"] == int(np.count_nonzero((mask != 0) & gr.members(g, of))) > 0
        check(v, want, of, gr.CHAMFER, mask, what="host mask")
    check(v, gr.geodesic_dijkstra(g, gr.EMPTY, gr.FACES, mask != 0), gr.EMPTY, gr.FACES, t.bool(), what="bool tensor")


def test_the_details_of_a_seed_list(writer):
    g = random_grid()
    v = writer
    lib, ctx = v._lib, v._ctx
    v.Voxelize(18)
    write_grid(v, g)
    m = gr.members(g, gr.EMPTY).reshape(-1)
    inside, outside = np.flatnonzero(m), np.flatnonzero(~m)
    plain = np.array([inside[5], inside[900], inside[-1]], np.uint32)
    want = gr.geodesic_dijkstra(g, gr.EMPTY, gr.CHAMFER, plain)
    _, info = check(v, want, gr.EMPTY, gr.CHAMFER, plain, what="list")
    assert info["seeds_used"] == 3
    _, info = check(v, want, gr.EMPTY, gr.CHAMFER, np.array([inside[5], inside[900], inside[5], inside[-1], inside[900]], np.uint32), what="duplicates")
    assert info["seeds_used"] == 3
    with_outsider = np.array([inside[5], outside[3], inside[-1]], np.uint32)
    _, info = check(v, gr.geodesic_dijkstra(g, gr.EMPTY, gr.CHAMFER, with_outsider), gr.EMPTY, gr.CHAMFER, with_outsider, what="a non-member among the seeds")
    assert info["seeds_used"] == 2                                      # one lower than the list is long
    nothing = np.where(m.reshape(g.shape), U, X).astype(np.uint32)
    _, info = check(v, nothing, gr.EMPTY, gr.CHAMFER, np.zeros(0, np.uint32), what="count 0")
    assert (info["rounds"], info["reached"], info["farthest"], info["farthest_voxel"]) == (1, 0, 0, 0xFFFFFFFF)
    assert lib.dxv_geodesic(ctx, 1, 1, 1, None, 0, 0) == 0              # count 0 with a NULL pointer
    before = v.GeodesicField()
    bad = np.array([inside[5], 18 ** 3], np.uint32)
    for fn in (lib.dxv_geodesic_async, lib.dxv_geodesic):
        assert fn(ctx, 1, 1, 1, bad.ctypes.data_as(C.c_void_p), 2, 0) == 1 and "outside the grid" in lib.dxv_last_error(ctx).decode()
    assert v.GeodesicField().tobytes() == before.tobytes()              # refused with nothing enqueued: the map of before is current and unchanged


def test_bytes_other_than_1_count_as_solid(writer):
    rng = np.random.default_rng(3)
    solid = random_grid() != 0
    g = np.where(solid, rng.integers(1, 256, solid.shape), 0).astype(np.uint8)
    assert len(np.unique(g)) > 100
    v = writer
    v.Voxelize(18)
    write_grid(v, g)
    for of in (gr.SOLID, gr.EMPTY):
        got, _ = check(v, gr.geodesic_dijkstra(solid.astype(np.uint8), of, gr.CHAMFER, "border"), of, gr.CHAMFER, "border", what="bytes")
        assert np.array_equal(got != X, gr.members(g, of))
    assert np.array_equal(v.Grid(), g)


# ---- frames, repeats, neighbours in the tool chain -----------------------------------------------------------------------------------------------
def test_two_frames_enqueued_back_to_back(dxv, bunny):
    vb, ib, _ = bunny
    v = dxv.Voxelizer(0)
    try:
        v.InitFromArrays(vb, ib)
        plan = [(0, 24, dxv.MODE_REFERENCE, gr.SOLID, gr.CHAMFER), (1, 18, dxv.MODE_SURFACE, gr.EMPTY, gr.FACES)]
        for frame, N, mode, of, metric in plan:                         # no synchronisation between any of these
            v.Voxelize(N, mode, sync=False, frameIndex=frame)
            assert v.Geodesic(of, metric, "border", sync=False) is True
        v.SyncAll()
        seen = set()
        for frame, N, mode, of, metric in plan:
            v.SetFrame(frame)
            v.Sync()
            g = v.Grid()
            want, tally, _ = gh.geodesic(g, of, metric, "border")
            assert g.any() and v.GeodesicField().tobytes() == want.tobytes(), frame
            info = v.GeodesicInfo()
            assert {k: info[k] for k in TALLY} == tally and info["ms"] > 0.0, frame
            seen.add(v.geodesic_device_ptr())
        assert len(seen) == 2
    finally:
        v.close()


def test_the_same_call_three_times_gives_the_same_bytes(writer, grids64):
    g = np.unpackbits(grids64["bunny_64_reference"])[: 64 ** 3].reshape(64, 64, 64).astype(np.uint8)
    v = writer
    v.Voxelize(64)
    write_grid(v, g)
    seeds = gr.smallest_member(g, gr.SOLID)
    want, _, _ = gh.geodesic(g, gr.SOLID, gr.CHAMFER, seeds)
    maps = [check(v, want, gr.SOLID, gr.CHAMFER, seeds, what="again")[0].tobytes() for _ in range(3)]
    assert maps[0] == maps[1] == maps[2]


def test_faces_from_the_border_reaches_exactly_what_the_fill_floods(dxv, writer):
    v = writer
    v.Voxelize(48, dxv.MODE_SURFACE)
    out = v.Geodesic(gr.EMPTY, gr.FACES, "border")
    shell = v.Grid()
    v.Fill(dxv.FILL_INTERIOR)
    interior = v.Grid()
    assert interior.any() and np.array_equal(out == U, interior != 0)   # unreached members == the fill's interior
    assert np.array_equal(out == X, shell != 0)


def test_the_path_on_the_bunny(writer, grids64):
    g = np.unpackbits(grids64["bunny_64_reference"])[: 64 ** 3].reshape(64, 64, 64).astype(np.uint8)
    v = writer
    v.Voxelize(64)
    write_grid(v, g)
    want, tally, _ = gh.geodesic(g, gr.SOLID, gr.CHAMFER, "border")
    _, info = check(v, want, gr.SOLID, gr.CHAMFER, "border", what="bunny")
    far = info["farthest_voxel"]
    p = v.GeodesicPath(far)
    gr.check_path(want, gr.CHAMFER, p, far)
    assert p.dtype == np.uint32 and p.tobytes() == gh.path(want, gr.CHAMFER, far).tobytes() and len(p) > 1
    lib, ctx = v._lib, v._ctx
    length, few = C.c_uint32(), np.full(3, 0xDEADBEEF, np.uint32)
    assert lib.dxv_geodesic_path(ctx, far, few.ctypes.data_as(C.c_void_p), 2, C.byref(length)) == 0
    assert length.value == len(p) and few.tolist() == [int(p[0]), int(p[1]), 0xDEADBEEF]        # min(length, capacity) indices are written
    seed = int(np.flatnonzero(want.reshape(-1) == 0)[0])
    assert v.GeodesicPath(seed).tolist() == [seed]
    for target, text in ((64 ** 3, "outside the grid"), (int(np.flatnonzero(g.reshape(-1) == 0)[0]), "holds no distance")):
        assert lib.dxv_geodesic_path(ctx, target, None, 0, C.byref(length)) == 1 and text in lib.dxv_last_error(ctx).decode()
    assert lib.dxv_geodesic_path(ctx, far, None, 4, C.byref(length)) == 1 and "NULL" in lib.dxv_last_error(ctx).decode()
    assert lib.dxv_geodesic_path(ctx, far, None, 0, None) == 1 and "length is NULL" in lib.dxv_last_error(ctx).decode()


def test_the_length_of_a_skeleton_by_the_double_sweep(dxv, writer):
    v = writer
    v.Voxelize(48, dxv.MODE_SURFACE)
    v.Fill()
    v.Thin(dxv.THIN_CURVE)
    g = v.Grid()
    assert g.any()
    first = gr.smallest_member(g, gr.SOLID)
    v.Geodesic(gr.SOLID, gr.CHAMFER, first)
    end = np.array([v.GeodesicInfo()["farthest_voxel"]], np.uint32)
    got, info = check(v, gr.geodesic_dijkstra(g, gr.SOLID, gr.CHAMFER, end), gr.SOLID, gr.CHAMFER, end, what="skeleton")
    p = v.GeodesicPath(info["farthest_voxel"])
    gr.check_path(got, gr.CHAMFER, p, info["farthest_voxel"])
    assert int(p[-1]) == int(end[0]) and info["farthest"] >= 3 * (len(p) - 1)


# ---- staleness, refusals, trim -----------------------------------------------------------------------------------------------------------------
def test_the_map_is_stale_once_the_grid_is_rewritten(dxv):
    from dxrvoxelizer_amd import meshes
    vb, ib = meshes.cube()
    v = dxv.Voxelizer(0)
    lib, ctx = v._lib, v._ctx

    def stale():
        with pytest.raises(dxv.DxvError, match="stale"):
            v.GeodesicField()
        with pytest.raises(dxv.DxvError, match="stale"):
            v.GeodesicInfo()
        with pytest.raises(dxv.DxvError, match="stale"):
            v.GeodesicPath(0)
        assert lib.dxv_geodesic_device_ptr(ctx) is None and "stale" in lib.dxv_last_error(ctx).decode()
        assert lib.dxv_geodesic_bytes(ctx) == 0
        buf = np.empty(16 ** 3, np.uint32)
        assert lib.dxv_geodesic_download(ctx, buf.ctypes.data_as(C.c_void_p), buf.nbytes) == 1 and "stale" in lib.dxv_last_error(ctx).decode()

    try:
        v.InitFromArrays(vb, ib)
        v.Voxelize(16, dxv.MODE_SURFACE)
        for edit in (lambda: v.Voxelize(16, dxv.MODE_SURFACE), lambda: v.Fill(), lambda: v.Morph(dxv.MORPH_ERODE, 1), lambda: v.Thin(dxv.THIN_CURVE),
                     lambda: (v.Components(gr.SOLID, 26), v.SelectComponents(dxv.SELECT_LARGEST)), lambda: (v.Octree(), v.OctreeExpand())):
            out = v.Geodesic(gr.SOLID, gr.CHAMFER, "border")
            assert (out < U).any() and lib.dxv_geodesic_bytes(ctx) == 4 * 16 ** 3
            v.Components(gr.EMPTY, 6)                                  # what only reads the grid leaves the map current
            v.Thickness(gr.SOLID, 9)
            assert v.GeodesicField().tobytes() == out.tobytes()
            edit()
            stale()
            v.Voxelize(16, dxv.MODE_SURFACE)
    finally:
        v.close()


def test_geodesic_refuses_with_a_message_and_leaves_everything_untouched(dxv):
    from dxrvoxelizer_amd import meshes
    vb, ib = meshes.tetrahedron()
    v = dxv.Voxelizer(0)
    lib, ctx = v._lib, v._ctx
    one = np.array([0], np.uint32)
    one_p = one.ctypes.data_as(C.c_void_p)

    def refused(args, text):
        for fn in (lib.dxv_geodesic_async, lib.dxv_geodesic):
            assert fn(ctx, *args) == 1 and text in lib.dxv_last_error(ctx).decode(), (text, lib.dxv_last_error(ctx).decode())

    try:
        refused((0, 1, 0, None, 0, 0), "no grid yet")                   # no launch
        assert lib.dxv_geodesic_device_ptr(ctx) is None and "no geodesic map yet" in lib.dxv_last_error(ctx).decode()
        assert lib.dxv_geodesic_bytes(ctx) == 0
        assert lib.dxv_geodesic_info(ctx, None, None, None, None, None, None, None) == 1 and "no geodesic map yet" in lib.dxv_last_error(ctx).decode()
        v.InitFromArrays(vb, ib)
        v.Voxelize(16)
        g = v.Grid()
        with pytest.raises(dxv.DxvError, match="no geodesic map yet"):
            v.GeodesicField()
        for of in (-1, 2):
            refused((of, 1, 0, None, 0, 0), "unknown kind")
        for metric in (-1, 2):
            refused((0, metric, 0, None, 0, 0), "unknown metric")
        for kind in (-1, 3):
            refused((0, 1, kind, None, 0, 0), "unknown seed kind")
        refused((0, 1, 1, None, 2, 0), "at NULL")
        refused((0, 1, 2, None, 0, 0), "seed mask is NULL")
        refused((0, 1, 2, one_p, 0, 0), "not device memory")            # a host pointer as a mask
        want = v.Geodesic(gr.SOLID, gr.CHAMFER, "border")
        refused((2, 1, 0, None, 0, 0), "unknown kind")                  # a refusal leaves the map of before current
        assert v.GeodesicField().tobytes() == want.tobytes() == gh.geodesic(g, gr.SOLID, gr.CHAMFER, "border")[0].tobytes()
        buf = np.empty(16 ** 3 + 1, np.uint32)                          # wrong download sizes
        assert lib.dxv_geodesic_download(ctx, buf.ctypes.data_as(C.c_void_p), buf.nbytes) == 1 and "expected" in lib.dxv_last_error(ctx).decode()
        assert lib.dxv_geodesic_download(ctx, None, 4 * 16 ** 3) == 1
        assert lib.dxv_geodesic_info(ctx, None, None, None, None, None, None, None) == 0
        assert np.array_equal(v.Grid(), g)
        v.Voxelize(16, z0=4, nz=8)                                      # a slab
        refused((0, 1, 0, None, 0, 0), "slab")
        v.Voxelize(952)                                                 # 5 (952^3 - 1) is beyond the codes; refused before anything is allocated
        refused((0, 1, 0, None, 0, 0), "0xFFFFFFFE")
        v.Voxelize(1026)
        refused((0, 0, 0, None, 0, 0), "at most 1024^3")
        assert lib.dxv_geodesic_bytes(ctx) == 0
    finally:
        v.close()


def test_after_trim_the_map_stays_and_the_call_works_again(dxv, bunny):
    vb, ib, _ = bunny
    v = dxv.Voxelizer(0)
    try:
        v.InitFromArrays(vb, ib)
        v.Voxelize(34)
        g = v.Grid()
        seeds = gr.smallest_member(g, gr.SOLID)
        want, tally, _ = gh.geodesic(g, gr.SOLID, gr.CHAMFER, seeds)
        check(v, want, gr.SOLID, gr.CHAMFER, seeds, what="before trim")
        v.trim()
        assert v.GeodesicField().tobytes() == want.tobytes()            # the map stays
        p = v.GeodesicPath(tally["farthest_voxel"])
        assert p.tobytes() == gh.path(want, gr.CHAMFER, tally["farthest_voxel"]).tobytes()
        check(v, want, gr.SOLID, gr.CHAMFER, seeds, what="after trim")
        check(v, gh.geodesic(g, gr.EMPTY, gr.FACES, "border")[0], gr.EMPTY, gr.FACES, "border", what="after trim")
        assert np.array_equal(v.Grid(), g)
    finally:
        v.close()


# ---- the C++ mirror ----------------------------------------------------------------------------------------------------------------------------
def test_cpp_mirror(dxv, bunny, tmp_path):
    vb, ib, _ = bunny
    np.ascontiguousarray(vb, np.float32).tofile(tmp_path / "vb.bin")
    np.ascontiguousarray(ib, np.uint32).tofile(tmp_path / "ib.bin")
    rocm = "/opt/rocm"
    exe = tmp_path / "geodesic_mirror"
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-D__HIP_PLATFORM_AMD__", "-I" + os.path.join(rocm, "include"),
                           os.path.join(ROOT, "tests", "cpp", "geodesic_mirror.cpp"), "-o", str(exe),
                           "-L" + os.path.join(ROOT, "dxrvoxelizer_amd"), "-l:libdxv.so", "-L" + os.path.join(rocm, "lib"), "-lamdhip64",
                           "-Wl,-rpath," + os.path.join(ROOT, "dxrvoxelizer_amd"), "-Wl,-rpath," + os.path.join(rocm, "lib")])
    r = subprocess.run([str(exe), str(tmp_path / "vb.bin"), str(tmp_path / "ib.bin"), "40", str(tmp_path / "map.bin"), str(tmp_path / "path.bin")], capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    v = dxv.Voxelizer(0)
    try:
        v.InitFromArrays(vb, ib)
        v.Voxelize(40)
        g = v.Grid()
    finally:
        v.close()
    lines = [[int(t) for t in line.split()] for line in r.stdout.splitlines()]
    assert len(lines) == 2
    first = gr.smallest_member(g, gr.SOLID)
    for line, (of, metric, seeds) in zip(lines, ((gr.EMPTY, gr.FACES, "border"), (gr.SOLID, gr.CHAMFER, first))):
        want, tally, _ = gh.geodesic(g, of, metric, seeds)
        assert line == [tally[k] for k in TALLY], (of, metric)
    assert np.fromfile(tmp_path / "map.bin", np.uint32).tobytes() == want.tobytes()
    assert np.fromfile(tmp_path / "path.bin", np.uint32).tobytes() == gh.path(want, gr.CHAMFER, tally["farthest_voxel"]).tobytes()
