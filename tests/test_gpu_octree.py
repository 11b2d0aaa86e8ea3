"""The sparse voxel octree on the GPU (include/dxv.h: dxv_octree*): the device's nodes and level table equal the numpy restatement
(tests/octree_restated.py) of the grid they were made from byte for byte -- arbitrary grids written through the frame's grid pointer, grids
smaller than a brick, cubes larger than their grid, meshes in three modes, a filled grid --, the expansion gives every voxel of the grid
back from the frame's own tree, from a caller's copy in another frame and in another context, three frames build side by side, the tree
goes stale when its grid changes, and the calls refuse what they must.
No malformed tree goes to the GPU: the checked descent is tested on the CPU (tests/test_octree_rule.py)."""
import ctypes as C

import numpy as np
import pytest

import octree_restated as orr
from raycast_restated import write_grid

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dxv(dxvlib):
    import dxrvoxelizer_amd
    return dxrvoxelizer_amd


def check(v, g, what):
    """the selected frame's tree against the restatement of grid g; returns the nodes"""
    nodes, first = v.Octree()
    want, wfirst = orr.build(g)
    N = g.shape[0]
    assert first == wfirst, (what, first, wfirst)
    assert nodes.dtype == np.uint32 and nodes.shape == want.shape and np.array_equal(nodes, want), what
    assert v.OctreeInfo() == (orr.levels_of(N), len(want), wfirst), what
    assert v.octree_bytes() == 8 * len(want) and v.octree_device_ptr(), what
    return nodes


def written_grids():
    rng = np.random.default_rng(7)
    for N in (2, 4, 6, 8, 16):
        yield f"random {N}", (rng.random((N, N, N)) < 0.5).astype(np.uint8)
    z, y, x = np.indices((8, 8, 8))
    yield "checkerboard 8", ((x + y + z) & 1).astype(np.uint8)
    yield "all solid 8", np.full((8, 8, 8), 0xFF, np.uint8)
    yield "all empty 8", np.zeros((8, 8, 8), np.uint8)
    one = np.zeros((8, 8, 8), np.uint8)
    one[7, 0, 3] = 1
    yield "one voxel 8", one
    slab = np.zeros((66, 66, 66), np.uint8)                             # S = 128: bricks that end inside the grid, guarded bytes
    slab[30:34, 20:23, 3:66] = 1
    yield "slab 66", slab
    for N in (2, 4, 6):
        yield f"all solid {N}", np.full((N, N, N), 7, np.uint8)
        yield f"all empty {N}", np.zeros((N, N, N), np.uint8)
    yield "ball 64", orr.ball(64, 31.9)                                 # full cells of several sizes
    big = (rng.random((72, 72, 72)) < 0.02).astype(np.uint8)            # S = 128: most of the cube lies outside the grid
    big[8:40, 16:48, 24:72] = 1
    yield "block and dust 72", big


GRIDS = list(written_grids())


@pytest.fixture(scope="module")
def writer(dxv, bunny):
    vb, ib, _ = bunny
    v = dxv.Voxelizer(0)
    v.InitFromArrays(vb, ib)
    yield v
    v.close()


@pytest.mark.parametrize("case", GRIDS, ids=[g[0] for g in GRIDS])
def test_written_grids_equal_restatement(dxv, writer, case):
    what, g = case
    v = writer
    v.Voxelize(g.shape[0])
    write_grid(v, g)
    nodes = check(v, g, what)
    if what == "all empty 8":
        assert [tuple(n) for n in nodes] == [(0, 0x0000)]
    if what == "all solid 8":
        assert [tuple(n) for n in nodes] == [(0, 0xFF00)]
    if what == "one voxel 8":
        assert [tuple(n) for n in nodes] == [(1, 0x0010), (2, 0x0020), (0, 0x2000)] and v.OctreeInfo()[2] == [0, 1, 2, 3]
    if what == "all solid 6":
        assert tuple(nodes[0]) == (1, 0x01FE) and v.OctreeInfo()[2] == [0, 1, 8, 8] and (nodes[1:, 1] & 0xFF == 0).all()
    assert v.octree_ms() > 0.0


@pytest.mark.parametrize("N", [16, 30])
@pytest.mark.parametrize("name", ["tetrahedron", "cube"])
def test_low_poly_meshes_in_parity_mode_equal_restatement(dxv, name, N):
    from dxrvoxelizer_amd import meshes
    vb, ib = getattr(meshes, name)()
    v = dxv.Voxelizer(0)
    try:
        v.InitFromArrays(vb, ib)
        v.Voxelize(N, dxv.MODE_PARITY)
        g = v.Grid()
        assert g.any()
        check(v, g, f"{name} {N}")
    finally:
        v.close()


def test_bunny_in_the_reference_rule_and_as_a_whole_at_256(dxv, writer):
    v = writer
    for N in (64, 256):
        v.Voxelize(N, dxv.MODE_REFERENCE)
        g = v.Grid()
        nodes = check(v, g, f"bunny {N}")
        assert 1 < len(nodes) < N ** 3 // 64
        print(f"bunny {N}: {len(nodes)} nodes, {8 * len(nodes)} bytes beside {v.grid_bytes()}, {v.octree_ms():.3f} ms")


def test_octree_of_a_filled_surface_describes_the_filled_grid(dxv, writer):
    v = writer
    v.Voxelize(32, dxv.MODE_SURFACE)
    shell = v.Grid()
    v.Fill()
    assert v.Octree(sync=False) is True                                 # behind the fill, nothing synchronised in between
    g = v.Grid()
    assert int((g != 0).sum()) > int((shell != 0).sum())
    nodes, first = v.OctreeNodes()
    want, wfirst = orr.build(g)
    assert first == wfirst and np.array_equal(nodes, want)
    v.Voxelize(32, dxv.MODE_REFERENCE_SURFACE)
    check(v, v.Grid(), "bunny 32 mode 3")


def as_device_words(nodes, offset_words=0):
    """a torch copy of the nodes on the device; offset_words = 1: four bytes into its allocation, so 4- but not 8-byte aligned"""
    import torch
    words = torch.from_numpy(np.ascontiguousarray(nodes, np.uint32).reshape(-1).view(np.int32))
    buf = torch.empty(words.numel() + offset_words, dtype=torch.int32, device="cuda")
    buf[offset_words:].copy_(words)
    torch.cuda.synchronize()
    return buf[offset_words:]


@pytest.mark.parametrize("N", [6, 30, 64])                            # guarded bytes below and above a brick; aligned stores
def test_round_trip_gives_every_voxel_back(dxv, writer, bunny, N):
    v = writer
    L = orr.levels_of(N)
    v.SetFrame(0)
    v.Voxelize(N)
    g = v.Grid()
    g[0, 0, :] = 0xC0                                                   # (bytes other than 0 and 1, up to the grid's corner)
    g[N - 1, N - 1, N - 1] = 2
    write_grid(v, g)
    want = (g != 0).astype(np.uint8)
    nodes, _ = v.Octree()
    write_grid(v, np.full((N, N, N), 0xAB, np.uint8))                   # poison: every voxel must be written
    v.OctreeExpand()
    assert np.array_equal(v.Grid(), want)
    with pytest.raises(dxv.DxvError, match="stale"):                    # the frame's own tree went stale with its grid
        v.OctreeInfo()
    # a caller's copy of the nodes, four bytes off an 8-byte boundary, into another frame of the same N
    copy = as_device_words(nodes, 1)
    assert copy.data_ptr() % 8 == 4
    v.Voxelize(N, frameIndex=1)
    write_grid(v, np.full((N, N, N), 0xAB, np.uint8))
    v.OctreeExpand(copy, levels=L)
    assert np.array_equal(v.Grid(), want)
    v.Sync()                                                            # (a well-formed tree: nothing to report)
    # ... and into another context on the same device, asynchronously
    vb, ib, _ = bunny
    w = dxv.Voxelizer(0)
    try:
        w.InitFromArrays(vb, ib)
        w.Voxelize(N, dxv.MODE_PARITY)
        write_grid(w, np.full((N, N, N), 0xAB, np.uint8))
        assert w.OctreeExpand(int(copy.data_ptr()), levels=L, count=len(nodes), sync=False) is True
        assert np.array_equal(w.Grid(), want)
        again, _ = w.Octree()                                           # built there again: the same tree
        assert np.array_equal(again, nodes)
    finally:
        w.close()
        v.SetFrame(0)


def test_three_frames_in_flight_each_get_their_own_tree(dxv, bunny):
    vb, ib, _ = bunny
    v = dxv.Voxelizer(0)
    try:
        v.InitFromArrays(vb, ib)
        plan = [(0, 16, dxv.MODE_REFERENCE), (1, 24, dxv.MODE_PARITY), (2, 12, dxv.MODE_SURFACE)]
        for frame, N, mode in plan:                                     # no synchronisation between any of these
            v.Voxelize(N, mode, sync=False, frameIndex=frame)
            assert v.Octree(sync=False) is True
        v.SyncAll()
        seen = set()
        for frame, N, mode in plan:
            v.SetFrame(frame)
            v.Sync()
            assert v.octree_ms() > 0.0, frame
            nodes, first = v.OctreeNodes()
            want, wfirst = orr.build(v.Grid())
            assert first == wfirst and np.array_equal(nodes, want) and len(want) > 1, frame
            seen.add(v.octree_device_ptr())
        assert len(seen) == 3
    finally:
        v.close()


def test_tree_is_stale_after_voxelize_fill_and_expand_and_trim_keeps_it(dxv):
    from dxrvoxelizer_amd import meshes
    vb, ib = meshes.cube()
    v = dxv.Voxelizer(0)
    lib, ctx = v._lib, v._ctx

    def stale():
        with pytest.raises(dxv.DxvError, match="stale"):
            v.OctreeInfo()
        assert lib.dxv_octree_device_ptr(ctx) is None and "stale" in lib.dxv_last_error(ctx).decode()
        assert lib.dxv_octree_bytes(ctx) == 0
        buf = np.empty((4, 2), np.uint32)
        assert lib.dxv_octree_download(ctx, buf.ctypes.data_as(C.c_void_p), buf.nbytes) == 1 and "stale" in lib.dxv_last_error(ctx).decode()
        with pytest.raises(dxv.DxvError, match="stale"):                # ... and it cannot be expanded from
            v.OctreeExpand()

    try:
        v.InitFromArrays(vb, ib)
        v.Voxelize(16, dxv.MODE_SURFACE)
        first = v.Octree()
        assert len(first[0]) > 1
        v.trim()                                                       # the scratch goes, the nodes stay
        again = v.OctreeNodes()
        assert np.array_equal(again[0], first[0]) and again[1] == first[1]
        after = v.Octree()                                             # ... and the next build is the same tree
        assert np.array_equal(after[0], first[0]) and after[1] == first[1]
        v.Fill()                                                       # the grid changed under the tree
        stale()
        filled = v.Octree()
        assert not np.array_equal(filled[0], first[0])
        v.OctreeExpand()                                               # written again, if with the same voxels
        stale()
        assert np.array_equal(v.Octree()[0], filled[0])
        v.Voxelize(16)                                                 # launched again
        stale()
    finally:
        v.close()


def test_octree_refuses_with_a_message_and_launches_nothing(dxv):
    import torch
    from dxrvoxelizer_amd import meshes
    vb, ib = meshes.tetrahedron()
    v = dxv.Voxelizer(0)
    lib, ctx = v._lib, v._ctx

    def last():
        return lib.dxv_last_error(ctx).decode()

    def build_refused(text):
        for fn in (lib.dxv_octree_async, lib.dxv_octree):
            assert fn(ctx) == 1 and text in last(), (text, last())

    def expand_refused(ptr, nodes, levels, text):
        for fn in (lib.dxv_octree_expand_async, lib.dxv_octree_expand):
            assert fn(ctx, ptr, nodes, levels) == 1 and text in last(), (text, last())

    try:
        build_refused("no grid yet")                                   # no scene, no grid
        expand_refused(None, 0, 0, "no grid yet")
        assert lib.dxv_octree_info(ctx, None, None, None) == 1 and "no octree yet" in last()
        assert lib.dxv_octree_device_ptr(ctx) is None and lib.dxv_octree_bytes(ctx) == 0
        v.InitFromArrays(vb, ib)
        v.Voxelize(16, z0=4, nz=8)
        build_refused("slab")
        expand_refused(None, 0, 0, "slab")
        v.VoxelizeInterleaved(16, 0, 2, 4)
        build_refused("share")
        expand_refused(None, 0, 0, "share")
        v.Voxelize(16)
        expand_refused(None, 0, 0, "no octree yet")                    # the frame's own tree: there is none
        g = v.Grid()
        nodes, _ = v.Octree()
        tree = as_device_words(nodes)
        ptr, n = C.c_void_p(tree.data_ptr()), len(nodes)
        assert n > 1
        expand_refused(ptr, n, 3, "levels")
        expand_refused(ptr, n, 5, "levels")
        expand_refused(ptr, 0, 4, "0 nodes")
        expand_refused(ptr, 0x7FFFFFFF, 4, "allocation")               # 16 GiB of nodes: more than the allocation behind the pointer holds
        expand_refused(C.c_void_p(tree.data_ptr() + 2), n - 1, 4, "aligned")
        host = np.ascontiguousarray(nodes)
        expand_refused(host.ctypes.data_as(C.c_void_p), n, 4, "not device memory")
        with pytest.raises(dxv.DxvError, match="levels"):
            v.OctreeExpand(tree)
        with pytest.raises(dxv.DxvError, match="count"):
            v.OctreeExpand(tree.data_ptr(), levels=4)
        with pytest.raises(dxv.DxvError, match="32-bit words"):
            v.OctreeExpand(torch.zeros(8, dtype=torch.uint8, device="cuda"), levels=4)
        assert np.array_equal(v.Grid(), g)                             # nothing was written
        assert np.array_equal(v.OctreeNodes()[0], nodes)               # ... and the tree is still current
        buf = np.empty((n + 1, 2), np.uint32)
        assert lib.dxv_octree_download(ctx, buf.ctypes.data_as(C.c_void_p), buf.nbytes) == 1 and f"expected {8 * n} bytes" in last()
        assert lib.dxv_octree_download(ctx, None, 8 * n) == 1
        assert lib.dxv_octree_ms(ctx, None) == 1
        assert lib.dxv_octree_expand(ctx, ptr, n, 4) == 0              # the same call with what it asks for
        assert np.array_equal(v.Grid(), (g != 0).astype(np.uint8))
    finally:
        v.close()
