"""The access radius and the intrusion map on the GPU (include/dxv.h: dxv_access*, dxv_intrusion*): the device's maps (uint32 per voxel), their
histograms and the tally equal, as bytes, what the rule gives for the grid -- by the restatements (tests/access_restated.py) and by the host
library (tests/access_host.py: the product's routines run serially, held to the restatements by tests/test_access_rule.py) -- on the smallest
shapes that still reach each mechanism: the ink bottle; its throat at every offset of a tile; a chamber raised twice, under three batch sizes;
a staircase connected at 26 only; random grids and the checkerboard; every member a seed; the geodesic's reached set; the cap identity; a grid
of members only; no usable seed; the call's discipline; the bunny at 64^3."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import access_host as ah
import access_restated as ar
from raycast_restated import write_grid

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TALLY = ("seeds_used", "reached", "unreached", "widest", "widest_voxel")
SOLID, EMPTY = ar.SOLID, ar.EMPTY


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


def load(v, g):
    v.Voxelize(g.shape[0])
    write_grid(v, g)


def check(v, g, of, connectivity, cap, seeds="border", intrusion=True, host_seeds=None, restated=True, what=""):
    """Access of the selected frame, which holds g: maps, histograms and tally against the host library and, with `restated`, forms (a) and
    (c); returns (A, I, info).  host_seeds: what `seeds` holds, where that is a device tensor."""
    hs = seeds if host_seeds is None else host_seeds
    want = ah.access(g, of, connectivity, cap, hs, intrusion)
    key = (what, of, connectivity, cap, intrusion)
    A, I = v.Access(of, connectivity, cap, seeds, intrusion)
    assert A.dtype == np.uint32 and A.shape == g.shape and A.tobytes() == want["A"].tobytes(), (key, int(np.count_nonzero(A != want["A"])))
    assert v.AccessHistogram().tobytes() == want["hist_a"].tobytes() == ar.histogram(A, cap).tobytes(), key
    if intrusion:
        assert I.dtype == np.uint32 and I.shape == g.shape and I.tobytes() == want["I"].tobytes(), (key, int(np.count_nonzero(I != want["I"])))
        assert v.IntrusionHistogram().tobytes() == want["hist_i"].tobytes() == ar.histogram(I, cap).tobytes(), key
    else:
        assert I is None
    info = v.AccessInfo()
    assert {k: info[k] for k in TALLY} == want["tally"], (key, info, want["tally"])
    if restated:
        assert A.tobytes() == ar.access(g, of, connectivity, cap, hs).tobytes(), key
        assert want["tally"] == ar.tally(g, of, A, hs), key
        if intrusion:
            assert I.tobytes() == ar.intrusion(g, of, A).tobytes(), key
    return A, I, info


# ---- the ink bottle -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("width", [1, 3])
def test_the_ink_bottle(writer, width):
    g, channel, chamber = ar.ink_bottle(16, width)
    v = writer
    load(v, g)
    R = ar.radius(g, EMPTY, 4096)
    for connectivity in (6, 26):
        A, I, info = check(v, g, EMPTY, connectivity, 4096, what=f"bottle {width}")
        room = (slice(5, 12), slice(5, 12), slice(6, 13))
        assert R[channel] == (1 if width == 1 else 4) and A[chamber] == R[channel] and A[room].max() == R[channel] and R[chamber] == 16
        W = v.Thickness(EMPTY, 4096)
        assert (I[room] <= W[room]).all() and I[room].max() == R[channel] < W[room].max() and I[chamber] == R[channel] < W[chamber] == 16
        assert (A <= R).all() and (A[A > 0] <= I[A > 0]).all() and (I <= W).all()
        assert info["unreached"] == 0 and info["reached"] == int((g == 0).sum()) and info["ms"] > 0.0


@pytest.mark.parametrize("axis", ["x", "z"])
def test_the_throat_at_every_offset_of_a_tile(writer, axis):
    v = writer
    v.Voxelize(24)
    for shift in range(8):
        g, channel, chamber = ar.ink_bottle(24, 1, shift if axis == "x" else 0, shift if axis == "z" else 0)
        write_grid(v, g)
        A, I, _ = check(v, g, EMPTY, 6, 65, restated=False, what=f"throat {axis} {shift}")
        assert A[chamber] == 1 and A[channel] == 1 and I[chamber] == 1 and int(A.max()) == 1
        A, _, _ = check(v, g, EMPTY, 26, 65, intrusion=False, restated=False, what=f"throat {axis} {shift}")
        assert A[chamber] == 1


# ---- rounds and batches ---------------------------------------------------------------------------------------------------------------------
def test_a_chamber_raised_twice_under_three_batch_sizes(dxv, writer):
    g, seed, chamber = ar.raised_twice()
    v = writer
    load(v, g)
    seeds = np.array([seed], np.uint32)
    try:
        maps = []
        for batch in (1, 2, 0):
            v.set_option("accessrounds", batch)
            A, I, info = check(v, g, EMPTY, 6, 4096, seeds, what=f"accessrounds {batch}")
            maps.append(A.tobytes() + I.tobytes())
            assert A[chamber] == 4 and ar.radius(g, EMPTY, 4096)[chamber] == 9 and A[3, 10, 3] == 1 and info["seeds_used"] == 1
            if batch == 1:
                assert info["rounds"] > 1, info                         # the corridor crosses six tile faces: no single round carries a word that far
            work = v.access_work_info()
            assert work["tiles_run"] >= work["most_live_tiles"] > 0
        assert maps[0] == maps[1] == maps[2]
        with pytest.raises(dxv.DxvError, match="accessrounds"):
            v.set_option("accessrounds", 65)
        with pytest.raises(dxv.DxvError, match="accessrounds"):
            v.set_option("accessrounds", -1)
    finally:
        v.set_option("accessrounds", 0)


def test_a_staircase_is_connected_at_26_only(writer):
    g = ar.staircase()
    v = writer
    load(v, g)
    members = int((g == 0).sum())
    A, I, info = check(v, g, EMPTY, 6, 4096, what="staircase 6")
    assert (info["reached"], info["unreached"], info["widest"], info["widest_voxel"]) == (1, members - 1, 1, 0) and A[9, 9, 9] == 0 and I[9, 9, 9] == 0
    A, I, info = check(v, g, EMPTY, 26, 4096, what="staircase 26")
    assert (info["reached"], info["unreached"], info["widest"]) == (members, 0, 1) and A[9, 9, 9] == 1 and I[9, 9, 9] == 1


def random_grid():
    import grid_sides as gs
    return dict(gs.grids(18))["random 0.3"]


@pytest.mark.parametrize("name", ["random 0.3", "checkerboard"])
def test_both_kinds_and_both_connectivities_from_the_border(writer, name):
    g = random_grid() if name == "random 0.3" else ar.checkerboard(18)
    v = writer
    load(v, g)
    for of in (SOLID, EMPTY):
        for connectivity in (6, 26):
            for intrusion in (True, False):
                A, I, info = check(v, g, of, connectivity, 65, intrusion=intrusion, what=name)
                assert np.array_equal(A > 0, ar.access_by_thresholds(g, of, connectivity, 65) > 0)


# ---- against the neighbouring operators ---------------------------------------------------------------------------------------------------
def test_with_every_member_a_seed_it_is_the_radius_and_the_thickness(dxv, writer):
    import torch
    g = random_grid()
    v = writer
    load(v, g)
    everything = torch.ones(18 ** 3, dtype=torch.uint8, device="cuda")
    d = v.DistanceField(dxv.DIST_SQ_I32)
    for of in (SOLID, EMPTY):
        for cap in (9, 4096):
            A, I, info = check(v, g, of, 26, cap, everything, host_seeds=np.ones(g.shape, np.uint8), what="every member")
            R = np.where((d < 0) if of == SOLID else (d > 0), np.minimum(np.abs(d.astype(np.int64)), cap), 0)
            assert np.array_equal(A, R) and info["seeds_used"] == info["reached"] == int(ar.members(g, of).sum()) and info["unreached"] == 0
            W = v.Thickness(of, cap)
            assert I.tobytes() == W.tobytes() and v.IntrusionHistogram().tobytes() == v.ThicknessHistogram().tobytes()


def test_the_reached_set_is_the_geodesics(dxv, writer):
    g = random_grid()
    v = writer
    load(v, g)
    inside = np.flatnonzero(ar.members(g, EMPTY).reshape(-1))
    for seeds in ("border", np.array([inside[5], inside[900]], np.uint32)):
        for of in (SOLID, EMPTY):
            for connectivity, metric in ((6, dxv.GEO_FACES), (26, dxv.GEO_CHAMFER)):
                A, _, _ = check(v, g, of, connectivity, 65, seeds, intrusion=False, what="reached set")
                G = v.Geodesic(of, metric, seeds)
                assert np.array_equal(A > 0, G < dxv.GEO_UNREACHED), (of, connectivity)


def test_the_cap_identity_holds_for_the_access_map(writer):
    g, _, _ = ar.ink_bottle(16, 3)
    g[13:16, :, :] = 0                                                  # a slab open to the border beside the bottle: radii up to 9
    v = writer
    load(v, g)
    full, _, _ = check(v, g, EMPTY, 6, 4096, what="cap 4096")
    assert full.max() > 5
    for cap in (2, 5, 65):
        A, _, _ = check(v, g, EMPTY, 6, cap, what=f"cap {cap}")
        assert np.array_equal(A, np.minimum(full, cap)), cap


@pytest.mark.parametrize("N", [16, 2])
def test_a_grid_of_members_only_reads_the_cap_everywhere(writer, N):
    v = writer
    for of, g in ((SOLID, np.full((N, N, N), 0x7F, np.uint8)), (EMPTY, np.zeros((N, N, N), np.uint8))):
        load(v, g)
        A, I, info = check(v, g, of, 6, 4096, restated=False, what="members only")
        assert (A == 4096).all() and (I == 4096).all() and v.IntrusionHistogram()[4096] == N ** 3
        assert (info["reached"], info["unreached"], info["widest"], info["widest_voxel"]) == (N ** 3, 0, 4096, 0)


def test_without_a_usable_seed_everything_reads_0(writer):
    g = random_grid()
    v = writer
    load(v, g)
    lib, ctx = v._lib, v._ctx
    members = int(ar.members(g, EMPTY).sum())
    outsiders = np.flatnonzero(g.reshape(-1) != 0)[:7].astype(np.uint32)
    for seeds in (np.zeros(0, np.uint32), outsiders):
        A, I, info = check(v, g, EMPTY, 26, 65, seeds, what="no seed")
        assert not A.any() and not I.any()
        assert (info["seeds_used"], info["reached"], info["unreached"], info["widest"], info["widest_voxel"], info["rounds"]) == (0, 0, members, 0, 0xFFFFFFFF, 1)
    assert lib.dxv_access(ctx, 1, 26, 65, 1, None, 0, 1) == 0           # count 0 with a NULL pointer


# ---- the call's discipline -----------------------------------------------------------------------------------------------------------------
def test_bytes_other_than_1_count_as_solid(writer):
    rng = np.random.default_rng(3)
    solid = random_grid() != 0
    g = np.where(solid, rng.integers(1, 256, solid.shape), 0).astype(np.uint8)
    assert len(np.unique(g)) > 100
    v = writer
    load(v, g)
    for of in (SOLID, EMPTY):
        A, I, _ = check(v, g, of, 26, 65, what="bytes")
        want = ah.access(solid.astype(np.uint8), of, 26, 65)
        assert A.tobytes() == want["A"].tobytes() and I.tobytes() == want["I"].tobytes()
    assert np.array_equal(v.Grid(), g)


def test_the_details_of_a_seed_list_and_a_mask_in_device_memory(writer):
    import torch
    g = random_grid()
    v = writer
    load(v, g)
    lib, ctx = v._lib, v._ctx
    m = ar.members(g, EMPTY).reshape(-1)
    inside, outside = np.flatnonzero(m), np.flatnonzero(~m)
    plain = np.array([inside[5], inside[900], inside[-1]], np.uint32)
    A, I, info = check(v, g, EMPTY, 26, 65, plain, what="list")
    assert info["seeds_used"] == 3
    B, J, info = check(v, g, EMPTY, 26, 65, np.array([inside[5], inside[900], inside[5], inside[-1], inside[900], inside[5]], np.uint32), what="duplicates")
    assert info["seeds_used"] == 3 and A.tobytes() == B.tobytes() and I.tobytes() == J.tobytes()
    _, _, info = check(v, g, EMPTY, 26, 65, np.array([inside[5], outside[3], inside[-1]], np.uint32), what="a non-member among the seeds")
    assert info["seeds_used"] == 2
    rng = np.random.default_rng(11)
    mask = (rng.random(g.shape) < 0.01).astype(np.uint8) * 0x80
    t = torch.from_numpy(mask).cuda()
    for of in (SOLID, EMPTY):
        _, _, info = check(v, g, of, 6, 65, t, host_seeds=mask, what="device mask")
        assert info["seeds_used"] == int(np.count_nonzero((mask != 0) & ar.members(g, of))) > 0
        check(v, g, of, 6, 65, mask, what="host mask")
    check(v, g, EMPTY, 26, 65, t.bool(), host_seeds=mask, what="bool tensor")
    before = v.AccessField()
    bad = np.array([inside[5], 18 ** 3], np.uint32)
    for fn in (lib.dxv_access_async, lib.dxv_access):
        assert fn(ctx, 1, 26, 65, 1, bad.ctypes.data_as(C.c_void_p), 2, 1) == 1 and "outside the grid" in lib.dxv_last_error(ctx).decode()
    assert v.AccessField().tobytes() == before.tobytes()                # refused with nothing enqueued: the maps of before are current and unchanged


def test_two_frames_enqueued_back_to_back(dxv, bunny):
    vb, ib, _ = bunny
    v = dxv.Voxelizer(0)
    try:
        v.InitFromArrays(vb, ib)
        plan = [(0, 24, dxv.MODE_REFERENCE, SOLID, 26, True), (1, 18, dxv.MODE_SURFACE, EMPTY, 6, True), (2, 16, dxv.MODE_REFERENCE, EMPTY, 26, False)]
        for frame, N, mode, of, connectivity, intrusion in plan:        # no synchronisation between any of these
            v.Voxelize(N, mode, sync=False, frameIndex=frame)
            assert v.Access(of, connectivity, 65, "border", intrusion, sync=False) is True
        v.SyncAll()
        seen = set()
        for frame, N, mode, of, connectivity, intrusion in plan:
            v.SetFrame(frame)
            v.Sync()
            g = v.Grid()
            want = ah.access(g, of, connectivity, 65, "border", intrusion)
            assert g.any() and v.AccessField().tobytes() == want["A"].tobytes(), frame
            if intrusion:
                assert v.IntrusionField().tobytes() == want["I"].tobytes() and v.IntrusionHistogram().tobytes() == want["hist_i"].tobytes(), frame
            info = v.AccessInfo()
            assert {k: info[k] for k in TALLY} == want["tally"] and info["ms"] > 0.0, frame
            seen.add(v.access_device_ptrs()[0])
        assert len(seen) == 3
    finally:
        v.close()


@pytest.fixture(scope="module")
def bunny64(grids64):
    return np.unpackbits(grids64["bunny_64_reference"])[: 64 ** 3].reshape(64, 64, 64).astype(np.uint8)


@pytest.mark.parametrize("of", [SOLID, EMPTY])
def test_the_bunny_at_64_three_times(writer, bunny64, of):
    v = writer
    load(v, bunny64)
    maps = []
    for _ in range(3):
        A, I, info = check(v, bunny64, of, 26, 65, restated=False, what="bunny")
        maps.append(A.tobytes() + I.tobytes())
    assert maps[0] == maps[1] == maps[2] and info["reached"] > 0


def test_the_maps_are_stale_once_the_grid_is_rewritten(dxv):
    from dxrvoxelizer_amd import meshes
    vb, ib = meshes.cube()
    v = dxv.Voxelizer(0)
    lib, ctx = v._lib, v._ctx

    def stale():
        for read in (v.AccessField, v.AccessHistogram, v.IntrusionField, v.IntrusionHistogram, v.AccessInfo, v.access_work_info, v.access_device_ptrs):
            with pytest.raises(dxv.DxvError, match="stale"):
                read()
        assert lib.dxv_access_device_ptr(ctx) is None and "stale" in lib.dxv_last_error(ctx).decode()
        assert lib.dxv_intrusion_device_ptr(ctx) is None and "stale" in lib.dxv_last_error(ctx).decode()
        assert lib.dxv_access_bytes(ctx) == lib.dxv_intrusion_bytes(ctx) == lib.dxv_access_histogram_bytes(ctx) == lib.dxv_intrusion_histogram_bytes(ctx) == 0
        buf = np.empty(16 ** 3, np.uint32)
        assert lib.dxv_access_download(ctx, buf.ctypes.data_as(C.c_void_p), buf.nbytes) == 1 and "stale" in lib.dxv_last_error(ctx).decode()

    try:
        v.InitFromArrays(vb, ib)
        v.Voxelize(16, dxv.MODE_SURFACE)
        for edit in (lambda: v.Voxelize(16, dxv.MODE_SURFACE), lambda: v.Fill(), lambda: v.Morph(dxv.MORPH_ERODE, 1), lambda: v.Thin(dxv.THIN_CURVE),
                     lambda: (v.Components(SOLID, 26), v.SelectComponents(dxv.SELECT_LARGEST)), lambda: (v.Octree(), v.OctreeExpand())):
            A, I = v.Access(SOLID, 26, 65)                              # (the cube's shell lies on the grid's border)
            assert A.any() and I.any() and lib.dxv_access_bytes(ctx) == lib.dxv_intrusion_bytes(ctx) == 4 * 16 ** 3 and lib.dxv_access_histogram_bytes(ctx) == 66 * 8
            v.Components(EMPTY, 6)                                     # what only reads the grid leaves the maps current
            v.Thickness(SOLID, 9)
            v.Geodesic(EMPTY, dxv.GEO_FACES)
            assert v.AccessField().tobytes() == A.tobytes() and v.IntrusionField().tobytes() == I.tobytes()
            edit()
            stale()
            v.Voxelize(16, dxv.MODE_SURFACE)
    finally:
        v.close()


def test_access_refuses_with_a_message_and_leaves_everything_untouched(dxv):
    from dxrvoxelizer_amd import meshes
    vb, ib = meshes.tetrahedron()
    v = dxv.Voxelizer(0)
    lib, ctx = v._lib, v._ctx
    one = np.array([0], np.uint32)
    one_p = one.ctypes.data_as(C.c_void_p)

    def refused(args, text):
        for fn in (lib.dxv_access_async, lib.dxv_access):
            assert fn(ctx, *args) == 1 and text in lib.dxv_last_error(ctx).decode(), (text, lib.dxv_last_error(ctx).decode())

    try:
        refused((0, 26, 65, 0, None, 0, 1), "no grid yet")              # no launch
        assert lib.dxv_access_device_ptr(ctx) is None and "no access map yet" in lib.dxv_last_error(ctx).decode()
        assert lib.dxv_access_bytes(ctx) == 0 and lib.dxv_intrusion_bytes(ctx) == 0
        assert lib.dxv_access_info(ctx, None, None, None, None, None, None, None) == 1 and "no access map yet" in lib.dxv_last_error(ctx).decode()
        v.InitFromArrays(vb, ib)
        v.Voxelize(16)
        g = v.Grid()
        with pytest.raises(dxv.DxvError, match="no access map yet"):
            v.AccessField()
        for of in (-1, 2):
            refused((of, 26, 65, 0, None, 0, 1), "unknown kind")
        for connectivity in (0, 18, 27):
            refused((0, connectivity, 65, 0, None, 0, 1), "neither 6 nor 26")
        for cap in (0, 1, 4097):
            refused((0, 26, cap, 0, None, 0, 1), "cap_sq")
        for kind in (-1, 3):
            refused((0, 26, 65, kind, None, 0, 1), "unknown seed kind")
        refused((0, 26, 65, 1, None, 2, 1), "at NULL")
        refused((0, 26, 65, 2, None, 0, 1), "seed mask is NULL")
        refused((0, 26, 65, 2, one_p, 0, 1), "not device memory")       # a host pointer as a mask
        A, I = v.Access(SOLID, 26, 65)
        refused((2, 26, 65, 0, None, 0, 1), "unknown kind")             # a refusal leaves the maps of before current
        want = ah.access(g, SOLID, 26, 65)
        assert v.AccessField().tobytes() == A.tobytes() == want["A"].tobytes() and v.IntrusionField().tobytes() == I.tobytes() == want["I"].tobytes()
        buf = np.empty(16 ** 3 + 1, np.uint32)                          # wrong download sizes
        for fn in (lib.dxv_access_download, lib.dxv_intrusion_download, lib.dxv_access_histogram_download, lib.dxv_intrusion_histogram_download):
            assert fn(ctx, buf.ctypes.data_as(C.c_void_p), buf.nbytes) == 1 and "expected" in lib.dxv_last_error(ctx).decode()
        assert lib.dxv_access_download(ctx, None, 4 * 16 ** 3) == 1
        assert lib.dxv_access_info(ctx, None, None, None, None, None, None, None) == 0
        assert lib.dxv_access_work_info(ctx, None, None, None) == 0
        # made without the intrusion map: its accessors fail with a message, the access map's work
        A2, none = v.Access(SOLID, 26, 65, intrusion=False)
        assert none is None and A2.tobytes() == A.tobytes() and v.AccessHistogram().tobytes() == want["hist_a"].tobytes()
        assert lib.dxv_intrusion_device_ptr(ctx) is None and "without its intrusion map" in lib.dxv_last_error(ctx).decode()
        assert lib.dxv_intrusion_bytes(ctx) == 0 and lib.dxv_intrusion_histogram_bytes(ctx) == 0
        for fn in (lib.dxv_intrusion_download, lib.dxv_intrusion_histogram_download):
            assert fn(ctx, buf.ctypes.data_as(C.c_void_p), 4 * 16 ** 3) == 1 and "without its intrusion map" in lib.dxv_last_error(ctx).decode()
        with pytest.raises(dxv.DxvError, match="without its intrusion map"):
            v.IntrusionField()
        assert v.access_device_ptrs()[1] is None
        assert np.array_equal(v.Grid(), g)
        v.Voxelize(16, z0=4, nz=8)                                      # a slab
        refused((0, 26, 65, 0, None, 0, 1), "slab")
        v.Voxelize(1026)
        refused((0, 6, 65, 0, None, 0, 0), "at most 1024^3")
        assert lib.dxv_access_bytes(ctx) == 0
    finally:
        v.close()


def test_after_trim_the_maps_stay_and_the_call_works_again(dxv, bunny):
    vb, ib, _ = bunny
    v = dxv.Voxelizer(0)
    try:
        v.InitFromArrays(vb, ib)
        v.Voxelize(34)
        g = v.Grid()
        A, I, _ = check(v, g, EMPTY, 26, 65, restated=False, what="before trim")
        hist = v.IntrusionHistogram()
        v.trim()
        assert v.AccessField().tobytes() == A.tobytes() and v.IntrusionField().tobytes() == I.tobytes() and v.IntrusionHistogram().tobytes() == hist.tobytes()
        check(v, g, EMPTY, 26, 65, restated=False, what="after trim")
        check(v, g, SOLID, 6, 9, intrusion=False, restated=False, what="after trim")
        assert np.array_equal(v.Grid(), g)
    finally:
        v.close()


def test_the_intrusion_curve_of_the_ink_bottle(dxv, writer):
    g, _, _ = ar.ink_bottle(16, 3)
    v = writer
    load(v, g)
    _, I = v.Access(EMPTY, 6, 4096)
    info = v.AccessInfo()
    diameter, share = dxv.intrusion_curve(v.IntrusionHistogram(), info["reached"] + info["unreached"])
    assert diameter.dtype == np.float32 and len(diameter) == len(share) == 4096 and diameter[0] == 1.0 and diameter[3] == 3.0
    members = int((g == 0).sum())
    assert share[0] == 1.0 and np.allclose(share, [(I >= t).sum() / members for t in range(1, 4097)]) and share[4] == 0.0      # nothing wider than the channel gets in


# ---- the C++ mirror --------------------------------------------------------------------------------------------------------------------------
def test_cpp_mirror(dxv, bunny, tmp_path):
    vb, ib, _ = bunny
    np.ascontiguousarray(vb, np.float32).tofile(tmp_path / "vb.bin")
    np.ascontiguousarray(ib, np.uint32).tofile(tmp_path / "ib.bin")
    rocm = "/opt/rocm"
    exe = tmp_path / "access_mirror"
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-D__HIP_PLATFORM_AMD__", "-I" + os.path.join(rocm, "include"),
                           os.path.join(ROOT, "tests", "cpp", "access_mirror.cpp"), "-o", str(exe),
                           "-L" + os.path.join(ROOT, "dxrvoxelizer_amd"), "-l:libdxv.so", "-L" + os.path.join(rocm, "lib"), "-lamdhip64",
                           "-Wl,-rpath," + os.path.join(ROOT, "dxrvoxelizer_amd"), "-Wl,-rpath," + os.path.join(rocm, "lib")])
    out = [str(tmp_path / n) for n in ("access.bin", "intrusion.bin", "access2.bin")]
    r = subprocess.run([str(exe), str(tmp_path / "vb.bin"), str(tmp_path / "ib.bin"), "40"] + out, capture_output=True, text=True, timeout=300)
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
    first = np.array([np.flatnonzero(g.reshape(-1))[0]] * 2, np.uint32)
    one = ah.access(g, EMPTY, 6, 65)
    two = ah.access(g, SOLID, 26, 4096, first, intrusion=False)
    assert lines[0] == [one["tally"][k] for k in TALLY] and lines[1] == [two["tally"][k] for k in TALLY] and two["tally"]["seeds_used"] == 1
    assert np.fromfile(out[0], np.uint32).tobytes() == one["A"].tobytes() and np.fromfile(out[1], np.uint32).tobytes() == one["I"].tobytes()
    assert np.fromfile(out[2], np.uint32).tobytes() == two["A"].tobytes()
