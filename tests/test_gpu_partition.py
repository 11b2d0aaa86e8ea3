"""The maximal-ball partition on the GPU (include/dxv.h: dxv_partition*): the device's labels (uint32 per voxel), table (32-byte records) and
throats (20-byte records) equal, as bytes, what the numpy restatement gives for the grid (tests/partition_restated.py, form (a), which
tests/test_partition_restated.py holds to the definition read literally) -- for the smallest grid, balls across brick faces, edges and corners,
reaches of one to eight bricks, the 16^3 level with a wholesale-accepted cell and a reach beyond the grid's edge, the longest chains of ties, a
plate and a rod of R = 1, noise with thousands of regions and throats, all-solid and all-empty grids, every partprune, with and without throats,
the committed bunny grid's hashes (tests/golden/partition_hashes.json, tests/gen_partition_fixtures.py), three frames in flight, after dxv_trim;
what the call must leave alone; what makes the product stale; what it refuses; and the C++ mirror."""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

import partition_host as ph
import partition_restated as pr
from conftest import GOLD
from raycast_restated import write_grid

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("labels", "table", "throats")


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


_WANT = {}


def restated(key, g, of, cap):
    """the restatement of a grid the tests share, made once and left unchanged"""
    if (key, of, cap) not in _WANT:
        _WANT[key, of, cap] = pr.partition(g, of, cap)
    return _WANT[key, of, cap]


def same(got, want, what):
    for a, b, name in zip(got, want, NAMES):
        assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes(), (what, name, len(a), len(b))


def check(v, g, of, cap, what, want=None):
    """Partition(of, cap) of the selected frame, which holds g, against the restatement; returns what the device gave"""
    want = pr.partition(g, of, cap) if want is None else want
    got = v.Partition(of, cap)
    same(got, want, (what, of, cap))
    ms, regions, throats, faces = v.PartitionInfo()
    assert (regions, throats, faces) == (len(want[1]), len(want[2]), int(want[2]["faces"].sum())), (what, of, cap)
    return got


def load(v, N, g):
    v.Voxelize(N)
    write_grid(v, g)


# ---- shapes ------------------------------------------------------------------------------------------------------------------------------------
def test_the_smallest_grid(writer):
    v = writer
    v.Voxelize(2)
    one = np.zeros((2, 2, 2), np.uint8)
    one[1, 1, 1] = 1
    hole = np.full((2, 2, 2), 0x40, np.uint8)                           # bytes other than 0 and 1 count as solid
    hole[0, 0, 0] = 0
    for name, g in (("one solid voxel at a corner", one), ("one empty voxel at a corner", hole), ("full", np.full((2, 2, 2), 0xFF, np.uint8))):
        write_grid(v, g)
        for of in (pr.SOLID, pr.EMPTY):
            for cap in (1, 5, 4096):
                check(v, g, of, cap, f"N = 2, {name}")
    labels, table, throats = v.Partition(pr.SOLID, 5)
    assert (labels == 1).all() and table["root"].tolist() == [0] and table["voxels"].tolist() == [8]


@pytest.mark.parametrize("N", [8, 12])
def test_balls_across_brick_faces_edges_and_corners(writer, N):
    v = writer
    for seed, density in ((1, 0.9), (2, 0.7)):
        g = pr.noise(N, density, seed) * 0x81
        load(v, N, g)
        for of in (pr.SOLID, pr.EMPTY):
            check(v, g, of, 5, f"N = {N}")


@pytest.fixture(scope="module")
def blobs40():
    return pr.balls(40, 3, count=8, rmax=12)


@pytest.mark.parametrize("cap", [17, 101])
def test_blobs_whose_reach_crosses_one_to_three_bricks(writer, blobs40, cap):
    v = writer
    load(v, 40, blobs40)
    for of in (pr.SOLID, pr.EMPTY):
        got = check(v, blobs40, of, cap, "blobs 40", restated("blobs40", blobs40, of, cap))
        assert int(got[1]["radius_sq"].max()) == cap                    # balls that reach the cap: across one brick at 17, across three at 101


@pytest.fixture(scope="module")
def ball72():
    return pr.ball_beside_blobs()


@pytest.mark.parametrize("of", [pr.SOLID, pr.EMPTY])
def test_a_ball_of_radius_30_beside_blobs_under_cap_1025(writer, ball72, of):
    v = writer
    load(v, 72, ball72)
    want = restated("ball72", ball72, of, 1025)
    v.set_option("partstages", 1)
    try:
        check(v, ball72, of, 1025, "ball 72", want)
        stages, cells, voxels = v.partition_stage_info()
    finally:
        v.set_option("partstages", 0)
    if of == pr.SOLID:
        assert int(want[1]["radius_sq"].max()) == 901                  # the ball's middle: its reach of 30 crosses the grid's edge at x = 50 + 30 and covers whole 16^3 cells
    assert (cells, voxels) == ph.partition(ball72, of, 1025)[3][1:]    # the device walked exactly the cells and voxels the header's search walks
    assert set(stages) == {"field", "keys", "search", "roots", "regions", "throats"} and all(t > 0.0 for t in stages.values())
    print(f"ball 72 of {of}: {stages}, {cells} cells, {voxels} voxels")


def test_the_longest_chains_of_ties(writer):
    g = np.ones((72, 72, 72), np.uint8)
    v = writer
    load(v, 72, g)
    labels, table, throats = v.Partition(pr.SOLID, 2)
    assert (labels == 1).all() and len(throats) == 0
    assert table.tobytes() == np.array([(0, 2, 72 ** 3, 0, [0, 0, 0], [71, 71, 71], 1)], pr.REGION).tobytes()


def test_a_plate_and_a_rod_one_voxel_thick(writer):
    v = writer
    for name, g in (("plate", pr.sheet(40)), ("rod", pr.rod(40))):
        load(v, 40, g)
        labels, table, throats = check(v, g, pr.SOLID, 17, name)
        assert table["radius_sq"].tolist() == [1] and table["root"].tolist() == [int(np.flatnonzero(g.reshape(-1))[0])] and len(throats) == 0     # every R is 1: the chains run by index to the first voxel
        check(v, g, pr.EMPTY, 17, f"round a {name}")


def test_noise_with_thousands_of_regions_and_throats(writer):
    g = pr.noise(40, 0.5, 7)
    v = writer
    load(v, 40, g)
    for of in (pr.SOLID, pr.EMPTY):
        labels, table, throats = check(v, g, of, 17, "noise 0.5")
        assert len(table) > 2000 and len(throats) > 2000


def test_all_solid_then_all_empty(writer):
    v = writer
    for byte in (0xFF, 0):
        g = np.full((24, 24, 24), byte, np.uint8)
        load(v, 24, g)
        for of in (pr.SOLID, pr.EMPTY):
            labels, table, throats = check(v, g, of, 4096, f"all {byte}")
            whole = (byte != 0) == (of == pr.SOLID)
            assert len(table) == (1 if whole else 0) and len(throats) == 0
            if whole:
                assert table["radius_sq"].tolist() == [4096] and table["root"].tolist() == [0]        # no voxel outside the members: every R is the cap
            else:
                lib, ctx = v._lib, v._ctx                               # K = 0: no table, no throats, no message
                assert lib.dxv_partition_table_device_ptr(ctx) is None and lib.dxv_partition_table_bytes(ctx) == 0
                assert lib.dxv_partition_throats_device_ptr(ctx) is None and lib.dxv_partition_throats_bytes(ctx) == 0
                assert lib.dxv_partition_labels_device_ptr(ctx) is not None and not labels.any()


# ---- options -----------------------------------------------------------------------------------------------------------------------------------
def test_every_partprune_gives_the_same_bytes_and_the_same_call_twice(dxv, writer, blobs40):
    v = writer
    load(v, 40, blobs40)
    try:
        for of in (pr.SOLID, pr.EMPTY):
            want = restated("blobs40", blobs40, of, 101)
            tested = []
            for prune in (0, 1, 2, 3):
                v.set_option("partprune", prune)
                v.set_option("partstages", 1)
                same(v.Partition(of, 101), want, ("partprune", prune, of))
                same(v.Partition(of, 101), want, ("again", prune, of))
                tested.append(v.partition_stage_info()[1:])
                v.set_option("partstages", 0)
                v.Partition(of, 101)
                assert v.partition_stage_info() == ({k: 0.0 for k in ("field", "keys", "search", "roots", "regions", "throats")}, 0, 0)      # nothing is measured unless asked
            assert tested[0][0] == 0 and tested[3][1] * 4 < tested[0][1], tested
        with pytest.raises(dxv.DxvError, match="partprune"):
            v.set_option("partprune", 4)
    finally:
        v.set_option("partprune", 3)
        v.set_option("partstages", 0)


def test_without_throats_the_same_labels_and_table_but_for_the_throats_word(dxv, writer, blobs40):
    v = writer
    load(v, 40, blobs40)
    lib, ctx = v._lib, v._ctx
    for of in (pr.SOLID, pr.EMPTY):
        want = restated("blobs40", blobs40, of, 17)
        labels, table, throats = v.Partition(of, 17, throats=False)
        assert throats is None and labels.tobytes() == want[0].tobytes()
        stripped = want[1].copy()
        stripped["throats"] = 0
        assert table.tobytes() == stripped.tobytes() and want[1]["throats"].any()
        assert v.PartitionInfo()[1:] == (len(table), 0, 0)
        assert lib.dxv_partition_throats_device_ptr(ctx) is None and "made without throats" in lib.dxv_last_error(ctx).decode()
        assert lib.dxv_partition_throats_bytes(ctx) == 0
        with pytest.raises(dxv.DxvError, match="made without throats"):
            v.PartitionThroats()
        same(v.Partition(of, 17), want, ("with throats again", of))


# ---- committed hashes ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag", ["solid/65", "empty/65", "solid/1025"])
def test_the_bunny_grid_equals_committed_hashes(writer, grids64, tag):
    with open(os.path.join(GOLD, "partition_hashes.json")) as fh:
        want = json.load(fh)
    g = np.unpackbits(grids64["bunny_64_reference"])[: 64 ** 3].reshape(64, 64, 64).astype(np.uint8)
    assert pr.sha(g) == want["grid_sha256"]
    kind, cap = tag.split("/")
    v = writer
    load(v, 64, g)
    labels, table, throats = v.Partition(pr.SOLID if kind == "solid" else pr.EMPTY, int(cap))
    row = want[tag]
    assert (pr.sha(labels), pr.sha(table), pr.sha(throats)) == (row["labels_sha256"], row["table_sha256"], row["throats_sha256"]), tag
    ms, regions, count, faces = v.PartitionInfo()
    assert (regions, count, faces) == (row["regions"], row["throats"], row["interface_faces"]) and ms > 0.0
    assert int(table["radius_sq"].max()) == row["largest_radius_sq"]
    print(f"bunny 64 {tag}: {ms:.3f} ms, {regions} regions, {count} throats")


# ---- what the call leaves alone ------------------------------------------------------------------------------------------------------------
def test_the_grid_and_products_made_before_stay_current_and_unchanged(dxv, writer, blobs40):
    v = writer
    load(v, 40, blobs40)
    field = v.DistanceField(dxv.DIST_SQ_I32)
    ptr = v.distance_device_ptr()
    W = v.Thickness(pr.SOLID, 26)
    comp_labels, comp_table = v.Components(pr.SOLID, 26)
    for of in (pr.SOLID, pr.EMPTY):
        check(v, blobs40, of, 17, "beside other products", restated("blobs40", blobs40, of, 17))
    assert np.array_equal(v.Grid(), blobs40)
    assert v.distance_device_ptr() == ptr and v.Distance().tobytes() == field.tobytes()
    assert v.ThicknessField().tobytes() == W.tobytes()
    assert np.array_equal(v.ComponentLabels(), comp_labels) and np.array_equal(v.ComponentTable(), comp_table)
    v.Thickness(pr.EMPTY, 9)                                            # ... and what only reads the grid leaves the partition current
    same((v.PartitionLabels(), v.PartitionTable(), v.PartitionThroats()), restated("blobs40", blobs40, pr.EMPTY, 17), "after a thickness")


def test_three_frames_in_flight_each_get_their_own_product(dxv, bunny):
    vb, ib, _ = bunny
    v = dxv.Voxelizer(0)
    try:
        v.InitFromArrays(vb, ib)
        plan = [(0, 32, dxv.MODE_REFERENCE, pr.SOLID, 17), (1, 24, dxv.MODE_PARITY, pr.EMPTY, 30), (2, 16, dxv.MODE_SURFACE, pr.SOLID, 4096)]
        for frame, N, mode, of, cap in plan:                            # no synchronisation of the frames between any of these
            v.Voxelize(N, mode, sync=False, frameIndex=frame)
            assert v.Partition(of, cap, sync=False) is True
        v.SyncAll()
        seen = set()
        for frame, N, mode, of, cap in plan:
            v.SetFrame(frame)
            v.Sync()
            g = v.Grid()
            assert g.any()
            same((v.PartitionLabels(), v.PartitionTable(), v.PartitionThroats()), pr.partition(g, of, cap), frame)
            assert v.PartitionInfo()[0] > 0.0
            seen.add(v.partition_device_ptrs()[0])
        assert len(seen) == 3
    finally:
        v.close()


def test_after_trim_the_product_stays_and_the_call_works_again(dxv, bunny):
    vb, ib, _ = bunny
    v = dxv.Voxelizer(0)
    try:
        v.InitFromArrays(vb, ib)
        v.Voxelize(34)
        g = v.Grid()
        want = pr.partition(g, pr.SOLID, 65)
        same(v.Partition(pr.SOLID, 65), want, "before trim")
        v.trim()
        same((v.PartitionLabels(), v.PartitionTable(), v.PartitionThroats()), want, "after trim")      # labels, table and throats stay
        check(v, g, pr.SOLID, 65, "again after trim", want)
        check(v, g, pr.EMPTY, 10, "after trim")
        assert np.array_equal(v.Grid(), g)
    finally:
        v.close()


# ---- staleness, refusals ---------------------------------------------------------------------------------------------------------------------
def test_the_product_is_stale_once_the_grid_is_rewritten(dxv):
    from dxrvoxelizer_amd import meshes
    vb, ib = meshes.cube()
    v = dxv.Voxelizer(0)
    lib, ctx = v._lib, v._ctx

    def stale():
        for read in (v.PartitionLabels, v.PartitionTable, v.PartitionThroats):
            with pytest.raises(dxv.DxvError, match="stale"):
                read()
        for ptr in (lib.dxv_partition_labels_device_ptr, lib.dxv_partition_table_device_ptr, lib.dxv_partition_throats_device_ptr):
            assert ptr(ctx) is None and "stale" in lib.dxv_last_error(ctx).decode()
        assert lib.dxv_partition_labels_bytes(ctx) == 0 and lib.dxv_partition_table_bytes(ctx) == 0 and lib.dxv_partition_throats_bytes(ctx) == 0
        buf = np.empty(16 ** 3, np.uint32)
        assert lib.dxv_partition_labels_download(ctx, buf.ctypes.data_as(C.c_void_p), buf.nbytes) == 1 and "stale" in lib.dxv_last_error(ctx).decode()
        assert v.PartitionInfo()[1:] == (0, 0, 0)

    try:
        v.InitFromArrays(vb, ib)
        v.Voxelize(16, dxv.MODE_SURFACE)
        for edit in (lambda: v.Voxelize(16, dxv.MODE_SURFACE), lambda: v.Fill(), lambda: v.Morph(dxv.MORPH_ERODE, 1), lambda: v.Thin(dxv.THIN_CURVE),
                     lambda: (v.Components(pr.SOLID, 26), v.SelectComponents(dxv.SELECT_LARGEST)), lambda: (v.Octree(), v.OctreeExpand())):
            labels, table, throats = v.Partition(pr.EMPTY, 9)
            assert labels.any() and lib.dxv_partition_labels_bytes(ctx) == 4 * 16 ** 3 and lib.dxv_partition_table_bytes(ctx) == 32 * len(table) > 0
            v.Components(pr.EMPTY, 6)                                  # what only reads the grid leaves the partition current
            assert v.PartitionLabels().tobytes() == labels.tobytes()
            edit()
            stale()
            v.Voxelize(16, dxv.MODE_SURFACE)
    finally:
        v.close()


def test_partition_refuses_with_a_message_and_leaves_everything_untouched(dxv):
    from dxrvoxelizer_amd import meshes
    vb, ib = meshes.tetrahedron()
    v = dxv.Voxelizer(0)
    lib, ctx = v._lib, v._ctx

    def refused(of, cap, text):
        for fn in (lib.dxv_partition_async, lib.dxv_partition):
            assert fn(ctx, of, cap, 1) == 1 and text in lib.dxv_last_error(ctx).decode(), (text, lib.dxv_last_error(ctx).decode())

    try:
        refused(0, 17, "no grid yet")                                   # no launch
        assert lib.dxv_partition_labels_device_ptr(ctx) is None and "no partition yet" in lib.dxv_last_error(ctx).decode()
        assert lib.dxv_partition_labels_bytes(ctx) == 0 and lib.dxv_partition_table_bytes(ctx) == 0 and lib.dxv_partition_throats_bytes(ctx) == 0
        v.InitFromArrays(vb, ib)
        v.Voxelize(16)
        g = v.Grid()
        with pytest.raises(dxv.DxvError, match="no partition yet"):
            v.PartitionLabels()
        for of in (-1, 2):
            refused(of, 17, "unknown kind")
        for cap in (0, 4097, 1 << 31):
            refused(0, cap, "cap_sq")
        want = pr.partition(g, pr.SOLID, 17)
        field = v.DistanceField(dxv.DIST_SQ_I32)
        same(v.Partition(pr.SOLID, 17), want, "tetrahedron")
        refused(2, 17, "unknown kind")                                  # a refusal leaves the partition of before current
        refused(0, 0, "cap_sq")
        same((v.PartitionLabels(), v.PartitionTable(), v.PartitionThroats()), want, "after refusals")
        assert v.Distance().tobytes() == field.tobytes()
        buf = np.empty(16 ** 3 + 1, np.uint32)                          # wrong download sizes
        assert lib.dxv_partition_labels_download(ctx, buf.ctypes.data_as(C.c_void_p), buf.nbytes) == 1 and "expected" in lib.dxv_last_error(ctx).decode()
        assert lib.dxv_partition_labels_download(ctx, None, 4 * 16 ** 3) == 1
        assert lib.dxv_partition_table_download(ctx, buf.ctypes.data_as(C.c_void_p), 32 * len(want[1]) + 32) == 1 and "expected" in lib.dxv_last_error(ctx).decode()
        assert lib.dxv_partition_throats_download(ctx, buf.ctypes.data_as(C.c_void_p), 20 * len(want[2]) + 20) == 1 and "expected" in lib.dxv_last_error(ctx).decode()
        assert lib.dxv_partition_stage_info(ctx, None, None, None) == 1 and "ms is NULL" in lib.dxv_last_error(ctx).decode()
        assert lib.dxv_partition_info(ctx, None, None, None, None) == 0
        assert np.array_equal(v.Grid(), g)
        v.Voxelize(16, z0=4, nz=8)                                      # a slab
        refused(0, 17, "slab")
        v.Voxelize(1026)                                                # beyond the operator's largest grid: refused before anything is allocated
        refused(0, 17, "at most 1024^3")
        assert lib.dxv_partition_labels_bytes(ctx) == 0
    finally:
        v.close()


# ---- the C++ mirror ----------------------------------------------------------------------------------------------------------------------------
def test_cpp_mirror(dxv, bunny, tmp_path):
    vb, ib, _ = bunny
    np.ascontiguousarray(vb, np.float32).tofile(tmp_path / "vb.bin")
    np.ascontiguousarray(ib, np.uint32).tofile(tmp_path / "ib.bin")
    rocm = "/opt/rocm"
    exe = tmp_path / "partition_mirror"
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-D__HIP_PLATFORM_AMD__", "-I" + os.path.join(rocm, "include"),
                           os.path.join(ROOT, "tests", "cpp", "partition_mirror.cpp"), "-o", str(exe),
                           "-L" + os.path.join(ROOT, "dxrvoxelizer_amd"), "-l:libdxv.so", "-L" + os.path.join(rocm, "lib"), "-lamdhip64",
                           "-Wl,-rpath," + os.path.join(ROOT, "dxrvoxelizer_amd"), "-Wl,-rpath," + os.path.join(rocm, "lib")])
    r = subprocess.run([str(exe), str(tmp_path / "vb.bin"), str(tmp_path / "ib.bin"), "48", "65", str(tmp_path / "labels.bin")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    v = dxv.Voxelizer(0)
    try:
        v.InitFromArrays(vb, ib)
        v.Voxelize(48)
        g = v.Grid()
    finally:
        v.close()
    lines = [[int(t) for t in line.split()] for line in r.stdout.splitlines()]
    assert len(lines) == 2
    for line, of in zip(lines, (pr.EMPTY, pr.SOLID)):
        labels, table, throats = pr.partition(g, of, 65)
        big = int(np.argmax(table["voxels"]))                           # (the first of the largest, as the program's strict compare takes it)
        assert line == [int(np.count_nonzero(labels)), len(table), len(throats), int(throats["faces"].sum()), int(table["voxels"][big]), int(table["radius_sq"][big]),
                        int(throats["neck_sq"].max()) if len(throats) else 0], of
    assert np.fromfile(tmp_path / "labels.bin", np.uint32).tobytes() == pr.partition(g, pr.SOLID, 65)[0].tobytes()
