"""The order of a PREPARED work queue (queue_order.hip): direction-major -- the queued bricks sorted by (heavy first, direction tile
of the brick's centre, start radius), whole tiles dealt round-robin to the eight queues.  The order is not part of the result: the
grids are byte-equal to the launch that builds its own queue (and to the golden vectors), the queue holds the same bricks once each,
no direction tile is shared between two queues' own shares, no queue runs a tile backwards, and two builds give the same queue.
Shapes: 16^3 bricks; a side that is no power of two; a side that is no multiple of 16 (the clear is a kernel of its own) or of 4
(bricks hang over the end); a block-cyclic share; a slab whose last brick layer is clamped; a queue shorter than its eight queues."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

TETRAHEDRON = (np.array([[1, 1, 1], [-1, -1, 1], [-1, 1, -1], [1, -1, -1]], np.float32),
               np.array([0, 1, 2, 0, 3, 1, 0, 2, 3, 1, 3, 2], np.uint32))

# name -> (mesh, grid side, partition): ("whole",), ("slab", z0, nz) or ("share", rank, world, zblock)
SHAPES = {
    "bunny-64": ("bunny", 64, ("whole",)),
    "bunny-48": ("bunny", 48, ("whole",)),
    "bunny-36": ("bunny", 36, ("whole",)),
    "bunny-64-rank-1-of-2": ("bunny", 64, ("share", 1, 2, 4)),
    "bunny-64-slab-of-30": ("bunny", 64, ("slab", 8, 30)),
    "tetrahedron-4": ("tetrahedron", 4, ("whole",)),
}


@pytest.fixture(scope="module")
def dxv(dxvlib):
    import dxrvoxelizer_amd
    return dxrvoxelizer_amd


def mesh(name, bunny):
    if name == "bunny":
        return bunny[0], bunny[1]
    pos, ib = TETRAHEDRON
    nrm = pos / np.linalg.norm(pos, axis=1, keepdims=True)
    return np.hstack([pos, nrm]).astype(np.float32), ib


def poison(v, value=0xAB):
    import torch
    from dxrvoxelizer_amd.slabs import device_grid_tensor
    v.Sync()
    device_grid_tensor(v, "cuda").fill_(value)
    torch.cuda.synchronize()


def prepare(v, N, part):
    if part[0] == "share":
        v.PrepareLaunchInterleaved(N, *part[1:])
    elif part[0] == "slab":
        v.PrepareLaunch(N, part[1], part[2])
    else:
        v.PrepareLaunch(N)


def launch(v, N, part, **kw):
    if part[0] == "share":
        v.VoxelizeInterleaved(N, *part[1:], **kw)
    elif part[0] == "slab":
        v.Voxelize(N, 0, part[1], part[2], **kw)
    else:
        v.Voxelize(N, **kw)


def prepared_queue(v, N, part, texels):
    """A prepared launch over poison: (grid, texels or None, the queue's counts)."""
    poison(v)
    launch(v, N, part)
    st = v.stats()
    assert st["plan_prepared"] == 1
    chk, order = v.plan_check(), v.queue_order()
    assert chk["violations"] == 0 and chk["duplicates"] == 0 and chk["queued_bricks"] == st["plan_bricks"], chk
    assert order["shared_tiles"] == 0 and order["descents"] == 0, order
    assert order["items"] == st["plan_bricks"] > 0, (order, st["plan_bricks"])
    return v.Grid().copy(), (v.Texels().copy() if texels else None), (order, st["plan_bricks"], st["plan_waves"])


# (the texel image -- its clear reads the same mask -- on one shape)
@pytest.mark.parametrize("shape,texels", [(s, False) for s in SHAPES] + [("bunny-64", True)])
def test_direction_major_queue_runs_the_same_bricks_to_the_same_grid(dxv, bunny, grids64, shape, texels):
    name, N, part = SHAPES[shape]
    vb, ib = mesh(name, bunny)
    v = dxv.Voxelizer(0)
    try:
        if texels:
            v.EnableTexels(True)
        v.InitFromArrays(vb, ib)
        v.set_option("prepared", 0)
        launch(v, N, part)                                     # the launch that builds its own queue, in Morton order
        base = v.stats()
        assert base["plan_prepared"] == 0 and base["plan_bricks"] > 0
        want, want_t = v.Grid().copy(), (v.Texels().copy() if texels else None)
        if shape == "bunny-64":
            assert np.array_equal(want, np.unpackbits(grids64["bunny_64_reference"])[: 64 ** 3].reshape(64, 64, 64))
        if shape == "tetrahedron-4":
            assert base["plan_bricks"] < 8                     # some of the eight queues are empty, ceil(total / 8) = 1
        v.set_option("prepared", 1)
        prepare(v, N, part)
        assert v.stats()["prepare_ms"] > 0.0
        grid, tex, counts = prepared_queue(v, N, part, texels)
        assert counts[1] == base["plan_bricks"]                # the same bricks ...
        assert np.array_equal(grid, want)                      # ... to the same bytes
        if texels:
            assert np.array_equal(tex, want_t)
        # a second build of the same queue (Init drops the first): the same grid, the same counts
        v.InitFromArrays(vb, ib)
        prepare(v, N, part)
        assert v.stats()["prepare_ms"] > 0.0
        grid2, tex2, counts2 = prepared_queue(v, N, part, texels)
        assert counts2 == counts and np.array_equal(grid2, want)
        if texels:
            assert np.array_equal(tex2, want_t)
        # all three frames read the one queue
        for f in range(v.FrameCount):
            v.SetFrame(f)
            launch(v, N, part, sync=False)                     # (allocates the frame's grid)
        v.SyncAll()
        for f in range(v.FrameCount):
            v.SetFrame(f)
            poison(v, 0x5A + f)
        for f in range(v.FrameCount):
            launch(v, N, part, sync=False, frameIndex=f)
        v.SyncAll()
        for f in range(v.FrameCount):
            v.SetFrame(f)
            assert v.stats()["plan_prepared"] == 1 and np.array_equal(v.Grid(), want), f
            if texels:
                assert np.array_equal(v.Texels(), want_t), f
    finally:
        v.close()
