"""The local thickness on the GPU (include/dxv.h: dxv_thickness*): the device's map (uint32 per voxel) and histogram equal, as bytes, what the
rule gives for the grid -- by the host library (tests/thickness_host.py: the product's routines run serially, held to the numpy restatement by
tests/test_thickness_rule.py), by the restatement itself where it is quick, and for sampled voxels by its per-voxel form -- for a ladder of caps,
across the morph's form switch, for pure paint, for the smallest grid, for single voxels, for bytes other than 0 / 1, under every thickcull,
against the device's own opening, for the committed bunny grid's hashes (tests/golden/thickness.json, tests/gen_thickness_fixtures.py), for three
frames in flight, after dxv_trim; what the call must leave alone; what makes the map stale; what it refuses; and the C++ mirror."""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

import grid_sides as gs
import morph_restated as mr
import thickness_host as th
import thickness_restated as tr
from conftest import GOLD
from raycast_restated import write_grid
from thickness_restated import CAP_LADDER, ladder_grid

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


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


def check(v, g, of, cap, what, want=None):
    """Thickness(of, cap) of the selected frame, which holds g: map and histogram against `want` (the host library's when None); returns the map"""
    if want is None:
        want = th.thickness(g, of, cap)[0]
    got = v.Thickness(of, cap)
    assert got.dtype == np.uint32 and got.shape == g.shape and got.tobytes() == want.tobytes(), (what, of, cap, int(np.count_nonzero(got != want)))
    hist = v.ThicknessHistogram()
    assert hist.dtype == np.uint64 and hist.tobytes() == tr.histogram(want, cap).tobytes(), (what, of, cap)
    return got


# ---- caps ------------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def ladder():
    return ladder_grid()


@pytest.mark.parametrize("cap", CAP_LADDER)
def test_cap_ladder_on_a_union_of_balls(writer, ladder, cap):
    v = writer
    v.Voxelize(40)
    write_grid(v, ladder)
    for of in (tr.SOLID, tr.EMPTY):
        W = check(v, ladder, of, cap, "ladder")
        assert int(W.max()) == cap
        centres, items = th.thickness(ladder, of, cap)[2]
        assert v.ThicknessInfo()[1:] == (centres, items)
        assert (centres == 0) == (cap == 2)


def big_ball_grid():
    """72^3: a ball of radius 33.5 round the middle -- depth 33 at its centre, so R reaches 1024 .. 1089 -- and five smaller ones"""
    z, y, x = np.indices((72, 72, 72))
    g = (z - 36) ** 2 + (y - 36) ** 2 + (x - 36) ** 2 <= 33.5 ** 2
    return (g | (tr.balls(72, 11, count=5, rmax=9) != 0)).astype(np.uint8)


@pytest.fixture(scope="module")
def big_ball():
    g = big_ball_grid()
    d2 = tr.radius(g, tr.SOLID, 1 << 30)                               # uncapped: the caps below take their minimum with it
    assert int(d2.max()) >= 33 * 33
    rng = np.random.default_rng(5)
    inside = np.argwhere(g != 0)
    points = [tuple(p) for p in inside[rng.choice(len(inside), 190, replace=False)]] + [tuple(p) for p in rng.integers(0, 72, (10, 3))]
    return g, d2, points


@pytest.mark.parametrize("cap", [1024, 1025, 1026, 4096])               # the Top stage's r2 = cap - 1 crosses the morph's form switch at 1024
def test_a_ball_of_radius_33_across_the_form_switch(writer, big_ball, cap):
    g, d2, points = big_ball
    v = writer
    v.Voxelize(72)
    write_grid(v, g)
    W = check(v, g, tr.SOLID, cap, "radius 33")
    assert int(W.max()) == min(cap, int(d2.max()))
    sampled = tr.thickness_at(g, tr.SOLID, cap, points, np.minimum(d2, cap))
    assert np.array_equal(sampled, np.array([W[p] for p in points], np.uint32)), cap
    assert (sampled > 0).sum() >= 190


def test_pure_paint_a_ball_of_radius_30_under_the_largest_cap(writer):
    z, y, x = np.indices((64, 64, 64))
    g = ((z - 32) ** 2 + (y - 32) ** 2 + (x - 32) ** 2 <= 900).astype(np.uint8)
    v = writer
    v.Voxelize(64)
    write_grid(v, g)
    W = check(v, g, tr.SOLID, 4096, "radius 30")
    assert int(W.max()) == 901 < 4096                                  # (the nearest empty voxel of the middle is (30, 1, 0) away.)  Top is empty: every value above 1 was painted
    assert v.ThicknessInfo()[1] > 0
    check(v, g, tr.EMPTY, 4096, "round a ball of radius 30")


def test_the_smallest_grid(writer):
    v = writer
    v.Voxelize(2)
    for name, g in gs.grids(2):
        write_grid(v, g)
        for of in (tr.SOLID, tr.EMPTY):
            for cap in (2, 6, 4096):
                check(v, g, of, cap, f"N = 2, {name}", tr.thickness(g, of, cap))


def test_one_solid_voxel_and_one_empty_voxel_at_a_corner(writer):
    v = writer
    one = np.zeros((16, 16, 16), np.uint8)
    one[5, 9, 15] = 1
    v.Voxelize(16)
    write_grid(v, one)
    W = check(v, one, tr.SOLID, 4096, "one voxel")
    assert W[5, 9, 15] == 1 and int(W.sum()) == 1
    assert v.ThicknessHistogram()[[0, 1]].tolist() == [16 ** 3 - 1, 1]
    full = np.ones((72, 72, 72), np.uint8)
    full[0, 0, 0] = 0
    v.Voxelize(72)
    write_grid(v, full)
    W = check(v, full, tr.SOLID, 4096, "a full grid but for a corner")
    assert W[0, 0, 0] == 0 and np.count_nonzero(W == 4096) == 72 ** 3 - 1      # every other voxel reads the cap
    W = check(v, full, tr.EMPTY, 4096, "the corner itself")
    assert W[0, 0, 0] == 1 and int(W.sum()) == 1


def test_bytes_other_than_0_and_1_count_as_solid(writer):
    rng = np.random.default_rng(3)
    solid = tr.balls(24, 9) != 0
    g = np.where(solid, rng.integers(1, 256, solid.shape), 0).astype(np.uint8)
    assert len(np.unique(g)) > 100
    v = writer
    v.Voxelize(24)
    write_grid(v, g)
    for of in (tr.SOLID, tr.EMPTY):
        W = check(v, g, of, 17, "bytes", tr.thickness(solid.astype(np.uint8), of, 17))
        assert np.array_equal(W != 0, tr.members(g, of))
    assert np.array_equal(v.Grid(), g)


def test_every_thickcull_gives_the_same_bytes_and_the_same_call_twice(writer, ladder):
    v = writer
    v.Voxelize(40)
    write_grid(v, ladder)
    try:
        painted = []
        for cull in (0, 1, 2, 3):
            v.set_option("thickcull", cull)
            for of in (tr.SOLID, tr.EMPTY):
                first = check(v, ladder, of, 17, f"thickcull {cull}")
                assert v.ThicknessInfo()[1:] == th.thickness(ladder, of, 17, cull)[2], (cull, of)
                again = v.Thickness(of, 17)
                assert again.tobytes() == first.tobytes(), (cull, of)
            painted.append(v.ThicknessInfo()[1])
        assert painted[3] < painted[1] < painted[0] and painted[3] < painted[2] < painted[0], painted
        with pytest.raises(dxv_error(v), match="thickcull"):
            v.set_option("thickcull", 4)
    finally:
        v.set_option("thickcull", 3)


def dxv_error(v):
    import dxrvoxelizer_amd
    return dxrvoxelizer_amd.DxvError


@pytest.mark.parametrize("N,cap", [(40, 5), (40, 17), (40, 101), (72, 1025), (72, 1026)])
def test_the_capped_part_is_the_devices_own_opening(dxv, writer, ladder, N, cap):
    g = ladder if N == 40 else big_ball_grid()
    v = writer
    v.Voxelize(N)
    write_grid(v, g)
    W = v.Thickness(tr.SOLID, cap)
    v.Morph(dxv.MORPH_OPEN, cap - 1)
    opened = v.Grid()
    assert np.array_equal(W == cap, opened != 0) and opened.any(), (N, cap)


# ---- committed hashes ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag", ["solid/65", "solid/4096", "empty/65", "empty/4096"])
def test_the_bunny_grid_equals_committed_hashes(writer, grids64, tag):
    with open(os.path.join(GOLD, "thickness.json")) as fh:
        want = json.load(fh)
    g = np.unpackbits(grids64["bunny_64_reference"])[: 64 ** 3].reshape(64, 64, 64).astype(np.uint8)
    assert tr.sha(g) == want["grid_sha256"]
    kind, cap = tag.split("/")
    v = writer
    v.Voxelize(64)
    write_grid(v, g)
    assert v.Thickness(tr.SOLID if kind == "solid" else tr.EMPTY, int(cap)) is not None
    assert v.thickness_stage_info() == ({k: 0.0 for k in ("field", "top", "cull", "select", "paint", "histogram")}, 0, 0)      # nothing is measured unless asked
    v.set_option("thickstages", 1)
    try:
        W = v.Thickness(tr.SOLID if kind == "solid" else tr.EMPTY, int(cap))
        tested_before = v.thickness_stage_info()[1]
        W = v.Thickness(tr.SOLID if kind == "solid" else tr.EMPTY, int(cap))      # again, into the scratch the call before left its counts in
    finally:
        v.set_option("thickstages", 0)
    hist = v.ThicknessHistogram()
    row = want[tag]
    assert tr.sha(W) == row["field_sha256"] and tr.sha(hist) == row["histogram_sha256"], tag
    assert int(W.max()) == row["max"] and int(np.flatnonzero(hist[1:])[0]) + 1 == row["minimum_wall"]
    ms, centres, items = v.ThicknessInfo()
    assert (centres, items) == (row["centres_painted"], row["work_items"]) and ms > 0.0
    stages, tested, sent = v.thickness_stage_info()
    assert 0 < sent <= tested and tested >= items                      # (a slice holds at least its centre column's voxel)
    # the paint's counters start at 0 in every call (what it tests depends on the items alone): the one assertion that fails when k_thick_select
    # stops zeroing them -- a second call into the same scratch then counts on top of the first
    assert tested == tested_before, (tested, tested_before)
    assert set(stages) == {"field", "top", "cull", "select", "paint", "histogram"} and all(t > 0.0 for t in stages.values()) and sum(stages.values()) <= ms * 1.01 + 0.01   # (disjoint pieces of the whole, up to the events' resolution)
    print(f"bunny 64 {tag}: {ms:.3f} ms, {centres} centres, {items} items, {stages}")


# ---- what the call leaves alone ------------------------------------------------------------------------------------------------------------
def test_the_grid_and_a_distance_field_made_before_stay_current_and_unchanged(dxv, writer, ladder):
    v = writer
    v.Voxelize(40)
    write_grid(v, ladder)
    for fmt in (dxv.DIST_SQ_I32, dxv.DIST_F32):
        field = v.DistanceField(fmt)
        ptr = v.distance_device_ptr()
        for of in (tr.SOLID, tr.EMPTY):
            check(v, ladder, of, 26, "beside a distance field")
        assert np.array_equal(v.Grid(), ladder)
        assert v.distance_device_ptr() == ptr and v.Distance().tobytes() == field.tobytes(), fmt
    labels, table = v.Components(tr.SOLID, 26)
    check(v, ladder, tr.SOLID, 9, "beside a labelling")
    assert np.array_equal(v.ComponentLabels(), labels) and np.array_equal(v.ComponentTable(), table)


def test_three_frames_in_flight_each_get_their_own_map(dxv, bunny):
    vb, ib, _ = bunny
    v = dxv.Voxelizer(0)
    try:
        v.InitFromArrays(vb, ib)
        plan = [(0, 32, dxv.MODE_REFERENCE, tr.SOLID, 17), (1, 24, dxv.MODE_PARITY, tr.EMPTY, 30), (2, 16, dxv.MODE_SURFACE, tr.SOLID, 4096)]
        for frame, N, mode, of, cap in plan:                            # no synchronisation between any of these
            v.Voxelize(N, mode, sync=False, frameIndex=frame)
            assert v.Thickness(of, cap, sync=False) is True
        v.SyncAll()
        seen = set()
        for frame, N, mode, of, cap in plan:
            v.SetFrame(frame)
            v.Sync()
            g = v.Grid()
            want, hist, counters = th.thickness(g, of, cap)
            assert g.any() and v.ThicknessField().tobytes() == want.tobytes() and v.ThicknessHistogram().tobytes() == hist.tobytes(), frame
            ms, centres, items = v.ThicknessInfo()
            assert ms > 0.0 and (centres, items) == counters, frame
            seen.add(v.thickness_device_ptr())
        assert len(seen) == 3
    finally:
        v.close()


def test_after_trim_the_map_stays_and_the_call_works_again(dxv, bunny):
    vb, ib, _ = bunny
    v = dxv.Voxelizer(0)
    try:
        v.InitFromArrays(vb, ib)
        v.Voxelize(66)
        g = v.Grid()
        want, hist, _ = th.thickness(g, tr.SOLID, 65)
        assert v.Thickness(tr.SOLID, 65).tobytes() == want.tobytes()
        v.trim()
        assert v.ThicknessField().tobytes() == want.tobytes() and v.ThicknessHistogram().tobytes() == hist.tobytes()      # map and histogram stay
        check(v, g, tr.SOLID, 65, "after trim", want)
        check(v, g, tr.EMPTY, 10, "after trim")
        assert np.array_equal(v.Grid(), g)
    finally:
        v.close()


# ---- staleness, refusals ---------------------------------------------------------------------------------------------------------------------
def test_the_map_is_stale_once_the_grid_is_rewritten(dxv):
    from dxrvoxelizer_amd import meshes
    vb, ib = meshes.cube()
    v = dxv.Voxelizer(0)
    lib, ctx = v._lib, v._ctx

    def stale():
        with pytest.raises(dxv.DxvError, match="stale"):
            v.ThicknessField()
        with pytest.raises(dxv.DxvError, match="stale"):
            v.ThicknessHistogram()
        assert lib.dxv_thickness_device_ptr(ctx) is None and "stale" in lib.dxv_last_error(ctx).decode()
        assert lib.dxv_thickness_bytes(ctx) == 0 and lib.dxv_thickness_histogram_bytes(ctx) == 0
        buf = np.empty(16 ** 3, np.uint32)
        assert lib.dxv_thickness_download(ctx, buf.ctypes.data_as(C.c_void_p), buf.nbytes) == 1 and "stale" in lib.dxv_last_error(ctx).decode()
        hist = np.empty(10, np.uint64)
        assert lib.dxv_thickness_histogram_download(ctx, hist.ctypes.data_as(C.c_void_p), hist.nbytes) == 1 and "stale" in lib.dxv_last_error(ctx).decode()

    try:
        v.InitFromArrays(vb, ib)
        v.Voxelize(16, dxv.MODE_SURFACE)
        for edit in (lambda: v.Voxelize(16, dxv.MODE_SURFACE), lambda: v.Fill(), lambda: v.Morph(dxv.MORPH_ERODE, 1), lambda: v.Thin(dxv.THIN_CURVE),
                     lambda: (v.Components(tr.SOLID, 26), v.SelectComponents(dxv.SELECT_LARGEST)), lambda: (v.Octree(), v.OctreeExpand())):
            W = v.Thickness(tr.SOLID, 9)
            assert W.any() and lib.dxv_thickness_bytes(ctx) == 4 * 16 ** 3 and lib.dxv_thickness_histogram_bytes(ctx) == 80
            v.Components(tr.EMPTY, 6)                                  # what only reads the grid leaves the map current
            assert v.ThicknessField().tobytes() == W.tobytes()
            edit()
            stale()
            v.Voxelize(16, dxv.MODE_SURFACE)
    finally:
        v.close()


def test_thickness_refuses_with_a_message_and_leaves_everything_untouched(dxv):
    from dxrvoxelizer_amd import meshes
    vb, ib = meshes.tetrahedron()
    v = dxv.Voxelizer(0)
    lib, ctx = v._lib, v._ctx

    def refused(of, cap, text):
        for fn in (lib.dxv_thickness_async, lib.dxv_thickness):
            assert fn(ctx, of, cap) == 1 and text in lib.dxv_last_error(ctx).decode(), (text, lib.dxv_last_error(ctx).decode())

    try:
        refused(0, 17, "no grid yet")                                   # no launch
        assert lib.dxv_thickness_device_ptr(ctx) is None and "no thickness map yet" in lib.dxv_last_error(ctx).decode()
        assert lib.dxv_thickness_bytes(ctx) == 0 and lib.dxv_thickness_histogram_bytes(ctx) == 0
        v.InitFromArrays(vb, ib)
        v.Voxelize(16)
        g = v.Grid()
        with pytest.raises(dxv.DxvError, match="no thickness map yet"):
            v.ThicknessField()
        for of in (-1, 2):
            refused(of, 17, "unknown kind")
        for cap in (0, 1, 4097, 1 << 31):
            refused(0, cap, "cap_sq")
        want = v.Thickness(tr.SOLID, 17)
        refused(2, 17, "unknown kind")                                  # a refusal leaves the map of before current
        refused(0, 1, "cap_sq")
        assert v.ThicknessField().tobytes() == want.tobytes() == th.thickness(g, tr.SOLID, 17)[0].tobytes()
        buf = np.empty(16 ** 3 + 1, np.uint32)                          # wrong download sizes
        assert lib.dxv_thickness_download(ctx, buf.ctypes.data_as(C.c_void_p), buf.nbytes) == 1 and "expected" in lib.dxv_last_error(ctx).decode()
        assert lib.dxv_thickness_download(ctx, None, 4 * 16 ** 3) == 1
        assert lib.dxv_thickness_histogram_download(ctx, buf.ctypes.data_as(C.c_void_p), 17 * 8) == 1 and "expected" in lib.dxv_last_error(ctx).decode()
        assert lib.dxv_thickness_stage_info(ctx, None, None, None) == 1 and "ms is NULL" in lib.dxv_last_error(ctx).decode()
        assert lib.dxv_thickness_info(ctx, None, None, None) == 0
        assert np.array_equal(v.Grid(), g)
        v.Voxelize(16, z0=4, nz=8)                                      # a slab
        refused(0, 17, "slab")
        v.Voxelize(1026)                                                # beyond the operator's largest grid: refused before anything is allocated
        refused(0, 17, "at most 1024^3")
        assert lib.dxv_thickness_bytes(ctx) == 0
    finally:
        v.close()


# ---- the C++ mirror ----------------------------------------------------------------------------------------------------------------------------
def test_cpp_mirror(dxv, bunny, tmp_path):
    vb, ib, _ = bunny
    np.ascontiguousarray(vb, np.float32).tofile(tmp_path / "vb.bin")
    np.ascontiguousarray(ib, np.uint32).tofile(tmp_path / "ib.bin")
    rocm = "/opt/rocm"
    exe = tmp_path / "thickness_mirror"
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-D__HIP_PLATFORM_AMD__", "-I" + os.path.join(rocm, "include"),
                           os.path.join(ROOT, "tests", "cpp", "thickness_mirror.cpp"), "-o", str(exe),
                           "-L" + os.path.join(ROOT, "dxrvoxelizer_amd"), "-l:libdxv.so", "-L" + os.path.join(rocm, "lib"), "-lamdhip64",
                           "-Wl,-rpath," + os.path.join(ROOT, "dxrvoxelizer_amd"), "-Wl,-rpath," + os.path.join(rocm, "lib")])
    r = subprocess.run([str(exe), str(tmp_path / "vb.bin"), str(tmp_path / "ib.bin"), "48", "65", str(tmp_path / "map.bin")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    v = dxv.Voxelizer(0)
    try:
        v.InitFromArrays(vb, ib)
        v.Voxelize(48)
        g = v.Grid()
    finally:
        v.close()
    lines = [line.split() for line in r.stdout.splitlines()]
    assert len(lines) == 2
    for line, of in zip(lines, (tr.EMPTY, tr.SOLID)):
        W, hist, counters = th.thickness(g, of, 65)
        wall = int(np.flatnonzero(hist[1:])[0]) + 1
        assert [int(line[0]), int(line[1]), int(line[2])] == [int(np.count_nonzero(W)), int(W.max()), wall], of
        assert abs(float(line[3]) - (2.0 * np.sqrt(wall) - 1.0)) < 1e-3 and (int(line[4]), int(line[5])) == counters
    assert np.fromfile(tmp_path / "map.bin", np.uint32).tobytes() == th.thickness(g, tr.SOLID, 65)[0].tobytes()
