"""Every launch path of the voxelizer at every even side 2 .. 72 and at 100, 130 and 194, on a mesh whose solid and empty voxels reach into all
three last brick layers (tests/launch_sides.py; the conditions are asserted there, on the oracle alone, and the host-compiled half of the
code is pinned to the same results by tests/test_launch_sides.py).  What only the device has, and what branches on a residue of the side N
or of a partition's height nz:
  store_brick            N & 3 != 0: a byte per lane; else a ballot turned into dword rows; rz < nz, vz < nz, vx < N guard the overhang
  brick_voxel_clamped    the lanes of an overhanging brick repeat the grid's last voxels: they scan, queue, help and hold a hit -- and store nothing
  the prepared launch    N & 15 == 0: the clear inside the dispatch (a nibble of the live mask per 16 bytes); else the clear kernel, whose
                         byte count is then no multiple of 16; the same split for the texel image
  plan_layout            the Morton bits are the brick counts' common power of two; the division path of brick_of_lin where they are none
  the parity rows        iy[k] clamped to N - 1 in blocks of 2 x 2 and 4 x 4 rows
  the tree walks         the early return for ix >= N || iy >= N || lz >= nz under all eight brick shapes

The protocol of tests/test_gpu_texels.py (its settings_of, proven and Run are reused): every compared launch follows a launch of the cube
into the same frame, side and partition -- a grid and an image without a single zero -- the image is read back in between, and the grid is
then poisoned through its device pointer.  Grid and image are compared by array_equal, no voxel left out.  The kept queue alone is not
poisoned: a frame whose pointer the caller holds never keeps its queue (dxv_policy.h: queue_policy), so that path runs on a Voxelizer of
its own whose pointer nobody ever asked for, over the cube's grid of ones.

The maps.  The automatic map of this mesh (128) is asked for with listres 0, the coarse one is 16 and the fine one 512: the mesh has
lists on all three (test_the_maps_of_the_sweep), and every launch of a lists' path is asserted to have run on them."""
import numpy as np
import pytest

import launch_sides as ls
from test_gpu_prepared import poison
from test_gpu_texels import ALL_PATHS, DEFAULTS, LIST_PATHS, WHOLE, Run, earlier_scene, launch, prepare, proven, settings_of, slices_of

pytestmark = pytest.mark.gpu

OPTIONS = dict(DEFAULTS, brick=4, rows=1, rowblock=0, plists=1, plistres=0)      # every option a test of this file sets, and its default
COARSE, FINE = 16, 512
GUARD = 0xC3

GROUPS = {f"{g[0]}..{g[-1]}": tuple(g) for g in (ls.SWEEP[i:i + 6] for i in range(0, len(ls.SWEEP), 6))}
GROUPS.update({str(N): (N,) for N in ls.WIDE})
MAP_SIDES = (2, 6, 18, 30, 34, 50, 66, 70, 100, 130)
BRICK_SIDES = (2, 6, 10, 14, 18, 30, 34, 66, 70)
SLAB_SIDES = {"6, 10": (6, 10), "18, 22": (18, 22), "30, 34": (30, 34), "36, 66": (36, 66)}
SHARES = ((6, 3, 2), (6, 3, 1), (10, 5, 2), (12, 3, 4), (20, 5, 4), (24, 3, 8), (36, 3, 4), (36, 9, 4), (40, 5, 8), (60, 5, 4), (72, 3, 8), (72, 9, 8))
FLIGHT = (30, 34, 36)

# The sides below 8 at which stats() cannot prove a path, and why.  A cap, not a measurement: test_every_path_at_every_side asserts that
# exactly these are unproven, and no side from 8 up may ever stand here.
UNPROVEN = {
}
assert all(N < 8 for _, N in UNPROVEN)


@pytest.fixture(scope="module")
def dxv(dxvlib):
    import dxrvoxelizer_amd
    return dxrvoxelizer_amd


@pytest.fixture(scope="module")
def voxes(dxv):
    """image: texel image on, the frame every compared launch of the reference rule writes into; kept: the same, its grid's pointer never
    handed out; plain: no image (the parity rule, the brick shapes)"""
    made = {"image": dxv.Voxelizer(0), "kept": dxv.Voxelizer(0), "plain": dxv.Voxelizer(0)}
    made["image"].EnableTexels(True)
    made["kept"].EnableTexels(True)
    try:
        yield made
    finally:
        for v in made.values():
            v.close()


@pytest.fixture(autouse=True)
def defaults_again(voxes):
    """every option a test set is back at its default when the test ends, also when it failed"""
    try:
        yield
    finally:
        for v in voxes.values():
            v.SetFrame(0)
            for k, val in OPTIONS.items():
                v.set_option(k, val)


def set_defaults(v):
    for k, val in OPTIONS.items():
        v.set_option(k, val)


def where(N, part, zs, got, want):
    """the first differing voxel: global (z, y, x), the two values, and whether it lies in a brick that hangs over the grid's (or the
    partition's) end"""
    lz, y, x = (int(i) for i in np.argwhere(got != want)[0])
    nz = len(zs)
    over = (N % 4 != 0 and max(y, x) >= ls.overhang(N)) or (nz % 4 != 0 and lz >= 4 * ((nz - 1) // 4))
    return f"first at (z, y, x) = ({zs[lz]}, {y}, {x}), local slice {lz}: got {int(got[lz, y, x]):#x}, wanted {int(want[lz, y, x]):#x}; " \
           f"{'in an overhanging brick' if over else 'in a whole brick'}"


def guard_tensor(v, N):
    """the N^3 bytes behind the frame's grid pointer, sized by a whole-grid launch at this side (as slabs.device_grid_tensor wraps them)"""
    import torch
    from dxrvoxelizer_amd.slabs import _DeviceBuffer
    return torch.as_tensor(_DeviceBuffer(v.grid_device_ptr(writable=True), N ** 3), device="cuda")


class SideRun(Run):
    """Run of test_gpu_texels.py for the sweep's mesh: the wanted pair is the side's, the grid is poisoned in front of the compared launch,
    a slab's launch must leave the bytes behind its partition alone, and a difference is reported with its first voxel"""

    def __init__(self, voxes, orc):
        super().__init__(voxes["image"], orc)
        self.voxes, self.unproven = voxes, []

    def differs(self, what, got, want, N=None, part=WHOLE):
        for name, g, w in (("grid", got[0], want[0]), ("image", got[1], want[1])):
            if g.shape != w.shape:
                self.bad.append(what + (name, g.shape, w.shape))
            elif not np.array_equal(g, w):
                self.bad.append(what + (name, f"{int((g != w).sum())} differ", where(N, part, slices_of(N, part), g, w)))

    def compare(self, path, opts, prep, N, part=WHOLE, guard=False):
        import torch
        v = self.voxes["kept" if path == "kept" else "image"]
        vb, ib = ls.mesh()
        w = ls.wanted(self.orc, N)
        zs = slices_of(N, part)
        want = (w.ref[0][zs], w.ref[1][zs])
        what = (f"path {path}", str(opts), f"side {N}", f"partition {part}")
        evb, eib, _, etex = earlier_scene(self.orc, N)
        etex = etex[zs]
        assert ((etex != 0) & (want[1] == 0)).any(), what                # an image left as it was found cannot pass
        set_defaults(v)
        v.InitFromArrays(evb, eib)
        if guard:
            v.Voxelize(N)                                               # the whole grid at this side: the buffer holds N^3 bytes from here on
        launch(v, N, part)
        for k, val in opts.items():
            v.set_option(k, val)
        v.InitFromArrays(vb, ib, gridDim=N if prep and part == WHOLE else 0)
        if prep and part != WHOLE:
            prepare(v, N, part)
        assert np.array_equal(v.Texels(), etex), what + ("the frame's image did not carry over",)
        if path != "kept":
            poison(v)
        behind = None
        if guard:
            ptr, whole = v.grid_device_ptr(writable=True), guard_tensor(v, N)
            behind = whole[N * N * len(zs):]
            behind.fill_(GUARD)
            torch.cuda.synchronize()
        launch(v, N, part)
        st = first = v.stats()
        self.differs(what, (v.Grid(), v.Texels()), want, N, part)
        if guard:
            assert v.grid_device_ptr(writable=True) == ptr, what + ("the frame's grid was allocated again",)
            if behind.numel() and not bool((behind == GUARD).all()):
                at = int(torch.nonzero(behind != GUARD)[0]) + N * N * len(zs)
                self.bad.append(what + (f"{int((behind != GUARD).sum())} bytes behind the partition written", f"first at byte {at} = (z, y, x) ({at // (N * N)}, {at // N % N}, {at % N}) of the buffer"))
        if path == "kept":                                              # (the first launch built the queue; its Sync read the lengths)
            v.Sync()
            launch(v, N, part)
            st = v.stats()
            self.differs(what + ("second launch",), (v.Grid(), v.Texels()), want, N, part)
        self.launches += 1
        if proven(path, st, first):
            self.took.setdefault(path, set()).add((N, part))
        else:
            self.unproven.append((N, part, str(opts), {k: st[k] for k in ("list_entries", "list_res", "plan_prepared", "plan_bricks", "plan_waves", "plan_ms", "redo_rays")}))
        return st


def parity_launch(run, v, opts, N, part=WHOLE, guard=False):
    """the parity rule's launch under `opts` into a poisoned grid against the wanted parity grid (no image in this mode)"""
    import torch
    zs = slices_of(N, part)
    want = ls.wanted(run.orc, N).parity[zs]
    what = ("parity rule", str(opts), f"side {N}", f"partition {part}")
    for k, val in opts.items():
        v.set_option(k, val)
    if guard:
        v.Voxelize(N, 1)
    launch_mode(v, N, part, 1)
    poison(v)
    behind = None
    if guard:
        ptr, whole = v.grid_device_ptr(writable=True), guard_tensor(v, N)
        behind = whole[N * N * len(zs):]
        behind.fill_(GUARD)
        torch.cuda.synchronize()
    launch_mode(v, N, part, 1)
    got = v.Grid()
    if got.shape != want.shape:
        run.bad.append(what + (got.shape, want.shape))
    elif not np.array_equal(got, want):
        run.bad.append(what + (f"{int((got != want).sum())} differ", where(N, part, zs, got, want)))
    if guard:
        assert v.grid_device_ptr(writable=True) == ptr, what + ("the frame's grid was allocated again",)
        if behind.numel() and not bool((behind == GUARD).all()):
            run.bad.append(what + (f"{int((behind != GUARD).sum())} bytes behind the partition written",))
    run.launches += 1


def launch_mode(v, N, part, mode):
    if part[0] == "slab":
        v.Voxelize(N, mode, part[1], part[2])
    elif part[0] == "share":
        v.VoxelizeInterleaved(N, *part[1:], mode=mode)
    else:
        v.Voxelize(N, mode)


# ---- the maps ----------------------------------------------------------------------------------------------------------------------------
def test_the_maps_of_the_sweep(voxes):
    """The sweep's mesh has lists on the automatic map, on 16 and on 512."""
    v = voxes["image"]
    vb, ib = ls.mesh()
    seen = {}
    for listres in (0, COARSE, FINE):
        set_defaults(v)
        v.set_option("lists", 2)
        v.set_option("listres", listres)
        v.InitFromArrays(vb, ib)
        v.Voxelize(34)
        st = v.stats()
        seen[listres] = (st["list_res"], st["list_entries"])
    print("maps of the sweep's mesh (list_res, list_entries):", seen)
    assert seen[0][1] > 0 and seen[COARSE][0] == COARSE and seen[COARSE][1] > 0 and seen[FINE][0] == FINE and seen[FINE][1] > 0, seen


# ---- a, b: every path at every side, whole grid, image on; the path proven ---------------------------------------------------------------
@pytest.mark.parametrize("group", list(GROUPS))
@pytest.mark.parametrize("path", ALL_PATHS)
def test_every_path_at_every_side(voxes, orc, path, group):
    """Every setting of `path` at every side of the group, the lists' paths on the automatic map; and proven(...) holds for every setting at
    every side from 8 up, and below 8 fails exactly where UNPROVEN says."""
    run = SideRun(voxes, orc)
    for N in GROUPS[group]:
        for opts, prep in settings_of(path):
            st = run.compare(path, opts, prep, N)
            if path in LIST_PATHS:
                assert st["list_entries"] > 0, (path, N, opts, "the automatic map refused the mesh")
    run.done()
    unproven = {N for N, _, _, _ in run.unproven}
    print(f"unproven {path}:", run.unproven)
    assert unproven == {N for p, N in UNPROVEN if p == path and N in GROUPS[group]}, (path, run.unproven)
    assert not [N for N in unproven if N >= 8]


@pytest.mark.parametrize("path", LIST_PATHS)
def test_coarse_and_fine_maps(voxes, orc, path):
    """The lists' paths on a coarse and a fine map (16: a brick looks into a texel or two; 512: into a patch of them) where bricks hang
    over the grid and above the map: on the lists, and on the map asked for."""
    run = SideRun(voxes, orc)
    for N in MAP_SIDES:
        for listres in (COARSE, FINE):
            for opts, prep in settings_of(path, listres):
                st = run.compare(path, opts, prep, N)
                assert st["list_entries"] > 0 and st["list_res"] == listres, (path, N, opts, st["list_entries"], st["list_res"])
    run.done()
    assert not [u for u in run.unproven if u[0] >= 8], run.unproven


# ---- c: the tree walks under every brick shape -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("brick", range(8))
def test_tree_walks_under_every_brick_shape(voxes, orc, brick):
    """lists = 0, the reference rule without the image, the four walks; and the parity rule's per-voxel kernels in the combinations of
    test_gpu_parity.test_every_kernel_variant_gives_the_same_grid that name this shape.  Every shape returns early for the voxels of its
    bricks that lie behind the grid's end."""
    v = voxes["plain"]
    vb, ib = ls.mesh()
    run = SideRun(voxes, orc)
    set_defaults(v)
    v.set_option("lists", 0)
    v.set_option("brick", brick)
    v.InitFromArrays(vb, ib)
    for N in BRICK_SIDES:
        want = ls.wanted(orc, N).ref[0]
        v.Voxelize(N)
        for opts, _ in settings_of("tree"):
            for k, val in opts.items():
                v.set_option(k, val)
            poison(v)
            v.Voxelize(N)
            got = v.Grid()
            assert v.stats()["list_entries"] == 0
            if not np.array_equal(got, want):
                run.bad.append((f"tree walk, brick {brick}", str(opts), f"side {N}", f"{int((got != want).sum())} differ", where(N, WHOLE, range(N), got, want)))
        v.set_option("queue", 1)
        v.set_option("wide", 2)
        for rows, queue, b in ((1, 1, 4), (0, 1, 4), (0, 0, 1), (0, 1, 0)):
            if b == brick:
                parity_launch(run, v, dict(rows=rows, queue=queue), N)
        v.set_option("rows", 1)
        v.set_option("queue", 1)
    run.done()


# ---- d: the parity rule ------------------------------------------------------------------------------------------------------------------
PARITY_SETTINGS = ([dict(rows=1, rowblock=rb, plists=0) for rb in (1, 2, 4)] + [dict(rows=0, queue=q) for q in (1, 0)] +
                   [dict(rows=1, rowblock=0, plists=2, plistres=r) for r in (16, 128)] + [dict(rows=1, rowblock=0, plists=0)])


@pytest.mark.parametrize("group", [g for g in GROUPS if GROUPS[g][0] in ls.SWEEP])
def test_parity_rule_at_every_side(voxes, orc, group):
    """The row kernel in blocks of 1, 2 x 2 and 4 x 4 rows (the rows of a block that hangs over are clamped to N - 1 and written again), the
    per-voxel kernels with and without the postponed leaves, the row lists on two maps (where the library builds them for this mesh: the
    grid is compared either way) and the rows without lists."""
    v = voxes["plain"]
    vb, ib = ls.mesh()
    run = SideRun(voxes, orc)
    for N in GROUPS[group]:
        for opts in PARITY_SETTINGS:
            set_defaults(v)
            v.InitFromArrays(vb, ib)
            parity_launch(run, v, opts, N)
    run.done()
    assert run.launches == len(GROUPS[group]) * len(PARITY_SETTINGS)


# ---- e: slabs ----------------------------------------------------------------------------------------------------------------------------
def slabs_of(N):
    """slabs (z0, nz) with every pair of residues (z0 % 4, nz % 4) that fits into N slices, one of a single slice, (1, N - 1), and one or
    more that end on the grid's last slice"""
    out = []
    for a in range(4):
        for b in range(4):
            z0 = a + 4 if (a + b) % 2 and a + 4 + (b or 4) <= N else a
            nz = b or 4
            if z0 + nz + 4 <= N and a % 2:
                nz += 4
            if z0 + nz <= N:
                out.append((z0, nz))
    for extra in ((N // 2, 1), (1, N - 1), (N - 3, 3), (N - 5, 5), (N - 1, 1)):
        if extra not in out:
            out.append(extra)
    return out


def test_the_slabs_cover_every_pair_of_residues():
    for N in sum(SLAB_SIDES.values(), ()):
        slabs = slabs_of(N)
        assert all(nz >= 1 and z0 >= 0 and z0 + nz <= N for z0, nz in slabs), (N, slabs)
        fits = {(a, b) for a in range(4) for b in range(4) if a + (b or 4) <= N}
        assert {(z0 % 4, nz % 4) for z0, nz in slabs} >= fits, (N, slabs)
        assert any(nz == 1 for _, nz in slabs) and (1, N - 1) in slabs and any(z0 + nz == N and z0 > 0 for z0, nz in slabs)
        assert len(slabs) == len(set(slabs))


@pytest.mark.parametrize("sides", list(SLAB_SIDES))
@pytest.mark.parametrize("path", ("prepared", "queue", "box", "tree", "parity rows"))
def test_slabs_at_ragged_sides(voxes, orc, path, sides):
    """Slices [z0, z0 + nz) of the wanted grid and image for every pair of residues of z0 and nz: the rows of a slab's last brick layer that
    lie behind nz are not stored (rz < nz, vz < nz), the clears end where the partition ends -- the bytes of the frame's buffer from
    N * N * nz up to N^3, filled with a known byte in front of every launch, are found unchanged -- and the buffer is the one the
    whole-grid launch at this side sized."""
    run = SideRun(voxes, orc)
    vb, ib = ls.mesh()
    for N in SLAB_SIDES[sides]:
        for z0, nz in slabs_of(N):
            part = ("slab", z0, nz)
            if path == "parity rows":
                v = voxes["plain"]
                for rb in (1, 2, 4):
                    set_defaults(v)
                    v.InitFromArrays(vb, ib)
                    parity_launch(run, v, dict(rows=1, rowblock=rb, plists=0), N, part, guard=True)
            else:
                for opts, prep in settings_of(path):
                    run.compare(path, opts, prep, N, part, guard=True)
    run.done()
    if path != "parity rows":
        assert not [u for u in run.unproven if u[0] >= 8], run.unproven


# ---- f: block-cyclic shares --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,world,zblock", SHARES)
def test_block_cyclic_shares_at_sides_no_multiple_of_16(voxes, orc, N, world, zblock):
    """Every rank's share through PrepareLaunchInterleaved and its launch, and through the queue a launch builds itself: each rank's image
    equals the wanted slices in the partition's order, and the ranks' grids put together by slabs.scatter_interleaved are the wanted grid."""
    from dxrvoxelizer_amd.slabs import interleaved_slices, scatter_interleaved
    assert N % 16 != 0
    w = ls.wanted(orc, N)
    run = SideRun(voxes, orc)
    for path, (opts, prep) in (("prepared", settings_of("prepared")[2]), ("queue", settings_of("queue")[0])):
        parts = []
        for rank in range(world):
            part = ("share", rank, world, zblock)
            assert slices_of(N, part) == list(interleaved_slices(N, rank, world, zblock))
            run.compare(path, opts, prep, N, part)
            parts.append((rank, run.voxes["image"].Grid().copy()))
        assert np.array_equal(scatter_interleaved(parts, N, world, zblock), w.ref[0]), (path, N, world, zblock)
    run.done()
    assert not [u for u in run.unproven if u[0] >= 8], run.unproven


# ---- g: three frames in flight at three sides --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prepared", (True, False))
def test_three_frames_in_flight_at_three_sides(voxes, orc, prepared):
    """Frames 0, 1, 2 launched at 30, 34 and 36 without a Sync in between, each into a poisoned grid over the cube's image; then SyncAll.
    Prepared, the three launches read three queues of one context; unprepared, each builds its own on its frame's stream."""
    v = voxes["image"]
    vb, ib = ls.mesh()
    run = SideRun(voxes, orc)
    set_defaults(v)
    try:
        for f, N in enumerate(FLIGHT):
            evb, eib, _, etex = earlier_scene(orc, N)
            v.InitFromArrays(evb, eib)
            v.Voxelize(N, frameIndex=f)
            assert np.array_equal(v.Texels(), etex)
        v.set_option("lists", 2)
        v.InitFromArrays(vb, ib)
        if prepared:
            for N in FLIGHT:
                v.PrepareLaunch(N)
        for f in range(len(FLIGHT)):
            v.SetFrame(f)
            poison(v, 0x5A + f)
        for f, N in enumerate(FLIGHT):
            v.Voxelize(N, sync=False, frameIndex=f)
        v.SyncAll()
        for f, N in enumerate(FLIGHT):
            v.SetFrame(f)
            st = v.stats()
            assert st["list_entries"] > 0 and st["plan_prepared"] == int(prepared) and st["plan_bricks"] > 0, (f, N, st)
            run.differs((f"frame {f}", f"side {N}", "prepared" if prepared else "unprepared"), (v.Grid(), v.Texels()), ls.wanted(orc, N).ref, N)
    finally:
        v.SetFrame(0)
    run.done()
