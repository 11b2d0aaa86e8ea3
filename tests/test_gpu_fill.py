"""The exterior flood fill on the GPU (include/dxv.h: dxv_fill*): after a fill every byte of the device's grid equals the numpy restatement
(tests/fill_restated.py) of the grid as it was before -- array_equal, no tolerance, both kinds -- for meshes in every mode, for arbitrary
grids written through the frame's grid pointer, through the settle path (option fillrounds = 1), for large grids against committed
hashes (tests/golden/fill.json, tests/gen_fill_fixtures.py), for three frames in flight; the frame state a fill must touch; and the
calls refuse what they must."""
import json
import os

import numpy as np
import pytest

import distance_restated as dr
import fill_restated as fr
from conftest import GOLD, load_mesh
from raycast_restated import write_grid
from test_gpu_configs import make, sha

pytestmark = pytest.mark.gpu

KINDS = (fr.SOLID, fr.INTERIOR)


@pytest.fixture(scope="module")
def dxv(dxvlib):
    import dxrvoxelizer_amd
    return dxrvoxelizer_amd


def check_fill(v, before, produce, what_for):
    """both kinds: `produce()` puts `before` back into the selected frame, Fill(kind), the grid against the restatement of `before`.
    Returns the outside set of `before`."""
    out = fr.outside(before)
    for kind in KINDS:
        produce()
        assert v.Fill(kind) is True
        got = v.Grid()
        assert got.dtype == np.uint8 and np.array_equal(got, fr.fill_from(before, out, kind)), (what_for, kind)
        assert v.CountSolid() == int(np.count_nonzero(got)), (what_for, kind)          # the other accessors see the filled grid
    return out


# ---- meshes ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,N,modes", [("bunny", 64, (0, 1, 2, 3)), ("dragon", 64, (0, 1, 2, 3)), ("turingbowl", 64, (0, 1, 2, 3)),
                                          ("bunny", 128, (2, 3))])
def test_fill_of_mesh_grids_equals_restatement(dxv, name, N, modes):
    vb, ib, _ = load_mesh(name)
    v = dxv.Voxelizer(0)
    try:
        v.InitFromArrays(vb, ib)
        for mode in modes:
            v.Voxelize(N, mode)
            before = v.Grid()
            assert before.any()
            out = check_fill(v, before, lambda: v.Voxelize(N, mode), f"{name} {N} mode {mode}")
            enclosed = int(np.count_nonzero(~out & (before == 0)))
            print(f"{name} {N} mode {mode}: walls {int(np.count_nonzero(before))}, enclosed {enclosed}, rounds {v.fill_info()[1]}")
            if mode == dxv.MODE_SURFACE:
                assert enclosed > 0, (name, N)                         # the surface of these assets encloses something: no empty comparison
    finally:
        v.close()


# ---- arbitrary grids ----------------------------------------------------------------------------------------------------------------
def arbitrary_grids(N):
    z, y, x = np.indices((N, N, N))
    for density in (0.3, 0.6, 0.68, 0.72, 0.95):
        yield f"random {density}", fr.random_walls(N, density, 1000 + N, bytes_other_than_one=True)
    if N >= 8:
        yield "maze", fr.maze(N)
    yield "all zero", np.zeros((N, N, N), np.uint8)
    yield "all 0xFF", np.full((N, N, N), 0xFF, np.uint8)
    yield "checkerboard", ((x + y + z) & 1).astype(np.uint8)
    one = np.zeros((N, N, N), np.uint8)
    one[N - 1, 0, N // 2] = 1
    yield "one voxel", one


@pytest.mark.parametrize("N", [64, 96, 2])                           # 96: rows of one and a half words; 2: the smallest grid, all border
def test_fill_of_arbitrary_grids_equals_restatement(dxv, bunny, N):
    vb, ib, _ = bunny
    v = dxv.Voxelizer(0)
    try:
        v.InitFromArrays(vb, ib)
        v.Voxelize(N)
        for what, g in arbitrary_grids(N):
            check_fill(v, g, lambda: write_grid(v, g), f"N = {N}, {what}")
    finally:
        v.close()


# ---- the settle path ----------------------------------------------------------------------------------------------------------------
def test_one_round_per_batch_gives_the_same_grids(dxv, bunny):
    vb, ib, _ = bunny
    v = dxv.Voxelizer(0)
    try:
        v.InitFromArrays(vb, ib)
        v.Voxelize(64)
        for what, g in (("maze", fr.maze(64)), ("random 0.68", fr.random_walls(64, 0.68, 5))):
            out = fr.outside(g)
            for kind in KINDS:
                grids, rounds = [], []
                for batch in (0, 1, 7):                                 # the default, the smallest batch, one that does not divide the rounds
                    v.set_option("fillrounds", batch)
                    write_grid(v, g)
                    v.Fill(kind)
                    grids.append(v.Grid())
                    rounds.append(v.fill_info()[1])
                print(f"{what} kind {kind}: rounds {rounds}")
                for got in grids:
                    assert np.array_equal(got, fr.fill_from(g, out, kind)), (what, kind)
                assert all(r > 1 for r in rounds), (what, rounds)       # (how many belongs to the algorithm)
        with pytest.raises(dxv.DxvError, match="fillrounds"):
            v.set_option("fillrounds", 65)
    finally:
        v.close()


def test_async_fill_then_async_field_is_the_field_of_the_filled_grid(dxv, bunny):
    vb, ib, _ = bunny
    v = dxv.Voxelizer(0)
    try:
        v.InitFromArrays(vb, ib)
        v.set_option("fillrounds", 1)                                  # the fill is still unsettled when the field is asked for
        v.Voxelize(64, dxv.MODE_SURFACE)
        before = v.Grid()
        v.Voxelize(64, dxv.MODE_SURFACE, sync=False)
        assert v.Fill(sync=False) is True
        assert v.DistanceField(dxv.DIST_SQ_I32, sync=False) is True
        v.Sync()
        filled = fr.fill(before)
        assert np.array_equal(v.Distance(), dr.distance_sq(filled))
        assert np.array_equal(v.Grid(), filled)
    finally:
        v.close()


# ---- large grids ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", ["bunny/256", "torus1m/512", "dragon9/512"])
def test_fill_of_large_grids_equals_committed_hashes(dxv, key):
    with open(os.path.join(GOLD, "fill.json")) as fh:
        want = json.load(fh)[key]
    with open(os.path.join(GOLD, "surface.json")) as fh:
        surface = json.load(fh)
    name, N = key.split("/")
    vb, ib = make(name)
    v = dxv.Voxelizer(0)
    try:
        v.InitFromArrays(vb, ib)
        for kind, tag in ((dxv.FILL_SOLID, "solid"), (dxv.FILL_INTERIOR, "interior")):
            v.Voxelize(int(N), dxv.MODE_SURFACE)
            grid_hash = sha(v.Grid())
            assert grid_hash == want["grid_sha256"], f"{key}: the grid is not the one the fixture's fill was made from"
            if key in surface:
                assert grid_hash == surface[key]["surface"]["sha256"], key
            v.Fill(kind)
            assert v.CountSolid() == want[tag]["count"], (key, tag)
            assert sha(v.Grid()) == want[tag]["sha256"], f"{key} {tag}: the count agrees but the grid's hash differs"
            print(f"{key} {tag}: {v.fill_info()}")
    finally:
        v.close()


def test_cube_at_1024_fills_the_whole_grid(dxv):
    from dxrvoxelizer_amd import meshes
    vb, ib = meshes.cube()
    v = dxv.Voxelizer(0)
    try:
        v.InitFromArrays(vb, ib)
        v.Voxelize(1024, dxv.MODE_SURFACE)
        assert 0 < v.CountSolid() < 1024 ** 3
        v.Fill()                                                       # the shell lies on the grid's border: nothing free is on the border
        assert v.CountSolid() == 1024 ** 3
        print("cube 1024:", v.fill_info())
    finally:
        v.close()


# ---- frames ------------------------------------------------------------------------------------------------------------------------
def test_three_frames_in_flight_each_get_their_own_fill(dxv, bunny):
    vb, ib, _ = bunny
    v = dxv.Voxelizer(0)
    try:
        v.InitFromArrays(vb, ib)
        plan = [(0, 64, dxv.MODE_SURFACE, dxv.FILL_SOLID), (1, 96, dxv.MODE_REFERENCE_SURFACE, dxv.FILL_INTERIOR), (2, 48, dxv.MODE_PARITY, dxv.FILL_SOLID)]
        before = {}
        for frame, N, mode, kind in plan:
            v.Voxelize(N, mode, frameIndex=frame)
            before[frame] = v.Grid()
        for frame, N, mode, kind in plan:                               # no synchronisation between any of these
            v.Voxelize(N, mode, sync=False, frameIndex=frame)
            assert v.Fill(kind, sync=False) is True
        v.SyncAll()
        for frame, N, mode, kind in plan:
            v.SetFrame(frame)
            v.Sync()
            ms, rounds = v.fill_info()
            assert ms > 0.0 and rounds >= 1, frame
            got = v.Grid()
            assert got.shape == (N, N, N) and np.array_equal(got, fr.fill(before[frame], kind)), frame
    finally:
        v.close()


# ---- frame state ---------------------------------------------------------------------------------------------------------------------
def test_a_kept_queue_drops_its_zeros_after_a_fill(dxv, bunny):
    import torch
    from dxrvoxelizer_amd.slabs import _DeviceBuffer
    vb, ib, _ = bunny
    v = dxv.Voxelizer(0)
    try:
        v.InitFromArrays(vb, ib)
        v.set_option("plan", 1)                                        # queue and zeros are kept while the frame's next launch is the same one
        v.Voxelize(64)
        v.Voxelize(64)
        first = v.Grid()
        assert not first[:8, :8, :8].any()
        # a closed shell in a corner no queued brick covers, written behind the library's back (through the READ-ONLY pointer, so the
        # frame is not marked as written to): the kept launch trusts the zeros it left there, and the shell survives it
        shell = np.zeros_like(first)
        shell[:8, :8, :8] = 1
        shell[1:7, 1:7, 1:7] = 0
        poked = first | shell
        t = torch.as_tensor(_DeviceBuffer(v.grid_device_ptr(writable=False), v.grid_bytes()), device="cuda")
        t.copy_(torch.from_numpy(poked.reshape(-1)))
        torch.cuda.synchronize()
        v.Voxelize(64)
        assert np.array_equal(v.Grid(), poked)
        # the same grid filled: the fill's 1s lie in those bricks too, and the launch behind a fill clears everything
        v.Fill()
        filled = v.Grid()
        assert np.array_equal(filled, fr.fill(poked)) and filled[1:7, 1:7, 1:7].all()
        v.Voxelize(64)
        assert np.array_equal(v.Grid(), first)
    finally:
        v.close()


def test_a_field_made_before_a_fill_is_stale_after_it(dxv, bunny):
    vb, ib, _ = bunny
    v = dxv.Voxelizer(0)
    try:
        v.InitFromArrays(vb, ib)
        v.Voxelize(64, dxv.MODE_SURFACE)
        v.DistanceField(dxv.DIST_SQ_I32)
        assert v.distance_device_ptr()
        v.Fill()
        with pytest.raises(dxv.DxvError, match="stale"):
            v.distance_device_ptr()
        assert np.array_equal(v.DistanceField(dxv.DIST_SQ_I32), dr.distance_sq(v.Grid()))
    finally:
        v.close()


def test_trim_gives_back_the_masks_and_the_next_fill_is_the_same(dxv, dragon):
    import torch
    vb, ib, _ = dragon
    v = dxv.Voxelizer(0)
    try:
        v.InitFromArrays(vb, ib)
        v.Voxelize(256, dxv.MODE_SURFACE)
        v.Fill()
        first = v.Grid()
        free0 = torch.cuda.mem_get_info()[0]
        v.trim()
        assert torch.cuda.mem_get_info()[0] - free0 >= 256 ** 3 // 4    # the two bit masks (4 MiB) went back
        assert np.array_equal(v.Grid(), first)                         # the grid stayed
        v.Voxelize(256, dxv.MODE_SURFACE)
        v.Fill()
        assert np.array_equal(v.Grid(), first)
    finally:
        v.close()


# ---- refusals ------------------------------------------------------------------------------------------------------------------------
def test_fill_refuses_with_a_message_and_launches_nothing(dxv, bunny):
    vb, ib, _ = bunny
    v = dxv.Voxelizer(0)
    lib, ctx = v._lib, v._ctx
    try:
        v.InitFromArrays(vb, ib)
        with pytest.raises(dxv.DxvError, match="no grid yet"):         # before any launch
            v.Fill()
        v.Voxelize(64, z0=16, nz=32)
        slab = v.Grid()
        with pytest.raises(dxv.DxvError, match="not a slab or a share"):
            v.Fill()
        assert lib.dxv_fill_async(ctx, 0) == 1 and "not a slab or a share" in lib.dxv_last_error(ctx).decode()
        assert np.array_equal(v.Grid(), slab)
        v.VoxelizeInterleaved(64, 1, 2, 8)
        share = v.Grid()
        with pytest.raises(dxv.DxvError, match="not a slab or a share"):
            v.Fill()
        assert np.array_equal(v.Grid(), share)
        v.Voxelize(64)
        whole = v.Grid()
        for bad in (-1, 2, 7):
            assert lib.dxv_fill_async(ctx, bad) == 1 and "unknown kind" in lib.dxv_last_error(ctx).decode()
            assert lib.dxv_fill(ctx, bad) == 1
        with pytest.raises(dxv.DxvError, match="unknown kind"):
            v.Fill(5)
        assert np.array_equal(v.Grid(), whole)                         # none of the refused calls touched the grid
        assert v.fill_info() == (0.0, 0)                               # ... or ran a round
        assert lib.dxv_fill_info(ctx, None, None) == 0
        v.Fill()
        assert np.array_equal(v.Grid(), fr.fill(whole)) and v.fill_info()[1] >= 1
    finally:
        v.close()
