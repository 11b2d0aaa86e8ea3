"""The texel image of the reference rule (EnableTexels: the packed interpolated normal of every inside hit, 0 elsewhere) against the
oracle on the meshes where kernels go wrong -- lattice meshes (rays through vertices, edges and coplanar duplicates: exact ties of t),
needles, and a sphere whose every triangle is there twice with other normals (a tie in every hit that only the image can see) --
through every launch path that computes it.  The grid is one bit of a hit; the image is thirty: the winner of a tie, the barycentrics,
the triangle whose normals were fetched.  Grid and image are compared by array_equal, no voxel left out.

The paths, and what in stats() proves that a launch took one (a launch that took another one -- a scene without lists walks the tree,
a scene without live bricks has no queue -- is compared all the same and counts for none):
  prepared   Init with the grid (or PrepareLaunch): k_voxelize_listed<true>, the hit in the LDS column; prepclear 0 .. 3 (a side that is
             a multiple of 16 clears the image inside the dispatch, any other through the clear kernel in front).  plan_prepared == 1.
  kept       plan = 1, dispatch = 1, the launch after the first one's Sync: the same kernel without any clear.  plan_waves is
             8 ceil(plan_bricks / 8) and not what the first launch ran.
  queue      no grid at Init, plan = 2: k_voxelize_queue<true>, the hit in registers; fuse 1 / 0, coop 1 / 0.  plan_bricks > 0,
             plan_ms > 0 (the queue was built inside the launch).
  box        plan = 0: k_voxelize<Brick<4, 4, 4>, 16, 0, true, 4> over the brick box; farmap 1 / 0.  list_entries > 0, no queue.
  tree       lists = 0: the walks, (queue, wide) = (1, 1), (1, 2), (1, 0), (0, 0).  list_entries == 0.
  redo       ... with a column of 8: the rays that run out of it are finished, image included, by k_voxelize_redo<0, true>.  redo_rays > 0.

There is no device pointer to poison the image through.  So every compared launch follows a launch of ANOTHER scene into the same frame
at the same side (the cube: an image without a single zero), the image is read back in between -- it must be the cube's: the buffer
carried over -- and the wanted image has zeros: a launch that leaves any part of the image as it found it fails.  (The kept queue's
second launch follows its own first by definition; the first follows the cube.)"""
import numpy as np
import pytest

from dxrvoxelizer_amd import meshes
from test_fuzz import CASES, doubled_sphere_wanted, lattice_mesh, needle_mesh

pytestmark = pytest.mark.gpu

# every option a path sets, and its default (dxv_policy.h): set back in front of every earlier launch and at the end
DEFAULTS = dict(lists=1, listres=0, plan=2, dispatch=1, prepared=1, prepclear=2, fuse=1, coop=1, farmap=1, queue=1, wide=2, stack=0)
WHOLE = ("whole",)
LIST_PATHS = ("prepared", "kept", "queue", "box")
ALL_PATHS = LIST_PATHS + ("tree", "redo")


@pytest.fixture(scope="module")
def dxv(dxvlib):
    import dxrvoxelizer_amd
    return dxrvoxelizer_amd


@pytest.fixture(scope="module")
def vox(dxv):
    """the one Voxelizer whose frame every launch of this file writes into, texel image on"""
    v = dxv.Voxelizer(0)
    v.EnableTexels(True)
    try:
        yield v
    finally:
        for k, val in DEFAULTS.items():
            v.set_option(k, val)
        v.EnableTexels(False)
        v.close()


# ---- the wanted pairs: computed once, shared, never written to ---------------------------------------------------------------------------
_EARLIER, _LATTICE, _SPHERE = {}, [], {}


def slices_of(N, part):
    """global slices of a partition, in the order its launch stores them"""
    if part[0] == "slab":
        return list(range(part[1], part[1] + part[2]))
    if part[0] == "share":
        r, world, zb = part[1:]
        return [z for z in range(N) if (z // zb) % world == r]
    return list(range(N))


def earlier_scene(orc, N):
    """the scene of the launch in front of every compared one: the cube, whose faces are the grid's -- every ray leaves through one of them,
    so its image is non-zero at EVERY voxel of these sides (the oracle's BVH: the image is only there to be overwritten, and recognised)"""
    if N not in _EARLIER:
        vb, ib = meshes.cube()
        grid, tex = orc.Scene(vb, ib).voxelize(N, texels=True)
        assert (tex != 0).all() and (grid != 0).all()
        _EARLIER[N] = (vb, ib, grid, tex)
    return _EARLIER[N]


def lattice_cases(orc):
    """(seed, n_tris, N, vb, ib, (grid, image), ties) of the lattice meshes as test_fuzz_gpu_vs_brute_force draws them, by the oracle's
    brute force.  ties: the image depends on which of two triangles hit at the same t wins -- with the triangles in the opposite order
    brute force gives another image."""
    if not _LATTICE:
        for seed, n_tris in CASES:
            rng = np.random.default_rng(1000 + seed)
            for N in (16, 32):
                vb, ib = lattice_mesh(rng, n_tris, N)
                want = orc.Scene(vb, ib).voxelize(N, algo=orc.ALGO_BRUTE, texels=True)
                assert np.array_equal(want[1] != 0, want[0] != 0)
                back = np.ascontiguousarray(ib.reshape(-1, 3)[::-1].reshape(-1))
                ties = not np.array_equal(orc.Scene(vb, back).voxelize(N, algo=orc.ALGO_BRUTE, texels=True)[1], want[1])
                _LATTICE.append((seed, n_tris, N, vb, ib, want, ties))
        assert sum(c[6] for c in _LATTICE) >= 6                         # (duplicates are one kind in six of the triangles drawn)
    return _LATTICE


# ---- one compared launch, over a stale image ---------------------------------------------------------------------------------------------
def launch(v, N, part):
    if part[0] == "slab":
        v.Voxelize(N, 0, part[1], part[2])
    elif part[0] == "share":
        v.VoxelizeInterleaved(N, *part[1:])
    else:
        v.Voxelize(N)


def prepare(v, N, part):
    if part[0] == "slab":
        v.PrepareLaunch(N, part[1], part[2])
    elif part[0] == "share":
        v.PrepareLaunchInterleaved(N, *part[1:])
    else:
        v.PrepareLaunch(N)


def settings_of(path, listres=0):
    """every setting a path is asked to run with: (options, prepare the partition)"""
    if path == "prepared":
        return [(dict(lists=2, listres=listres, prepclear=c), True) for c in (0, 1, 2, 3)]
    if path == "kept":
        return [(dict(lists=2, listres=listres, plan=1, dispatch=1), False)]
    if path == "queue":
        return [(dict(lists=2, listres=listres, plan=2, fuse=f, coop=c), False) for f in (1, 0) for c in (1, 0)]
    if path == "box":
        return [(dict(lists=2, listres=listres, plan=0, farmap=f), False) for f in (1, 0)]
    if path == "tree":
        return [(dict(lists=0, queue=q, wide=w), False) for q, w in ((1, 1), (1, 2), (1, 0), (0, 0))]
    assert path == "redo"
    return [(dict(lists=0, stack=8), False)]


def proven(path, st, first=None):
    """the launch took `path`: what its stats prove (module docstring)"""
    lists, bricks = st["list_entries"] > 0, st["plan_bricks"]
    if path == "prepared":
        return lists and st["plan_prepared"] == 1 and bricks > 0
    if path == "kept":
        return lists and st["plan_prepared"] == 0 and bricks > 0 and st["plan_waves"] == 8 * ((bricks + 7) // 8) != first["plan_waves"]
    if path == "queue":
        return lists and st["plan_prepared"] == 0 and bricks > 0 and st["plan_ms"] > 0.0
    if path == "box":
        return lists and st["plan_prepared"] == 0 and bricks == 0 and st["plan_waves"] == 0
    if path == "tree":
        return not lists and bricks == 0
    return not lists and st["redo_rays"] > 0


class Run:
    """the compared launches of one test: what differed from the oracle, and which paths were proven on which scenes"""

    def __init__(self, v, orc):
        self.v, self.orc, self.bad, self.took, self.launches = v, orc, [], {}, 0

    def differs(self, what, got, want):
        for name, g, w in (("grid", got[0], want[0]), ("image", got[1], want[1])):
            if g.shape != w.shape or not np.array_equal(g, w):
                self.bad.append(what + (name, int((g != w).sum()) if g.shape == w.shape else g.shape))

    def compare(self, what, path, opts, prep, vb, ib, N, want, part=WHOLE, tag=None):
        """The cube into the frame; then the scene under `opts`, the frame's image read back in front of its launch; the launch against
        `want`.  Returns the stats of the compared launch (of the kept queue: of its second launch)."""
        v = self.v
        zs = slices_of(N, part)
        want = (want[0][zs], want[1][zs])
        evb, eib, _, etex = earlier_scene(self.orc, N)
        etex = etex[zs]
        assert ((etex != 0) & (want[1] == 0)).any(), what                # an image left as it was found cannot pass
        for k, val in DEFAULTS.items():
            v.set_option(k, val)
        v.InitFromArrays(evb, eib)
        launch(v, N, part)
        for k, val in opts.items():
            v.set_option(k, val)
        v.InitFromArrays(vb, ib, gridDim=N if prep and part == WHOLE else 0)
        if prep and part != WHOLE:
            prepare(v, N, part)
        assert np.array_equal(v.Texels(), etex), what + ("the frame's image did not carry over",)
        launch(v, N, part)
        st = first = v.stats()
        self.differs(what + (path, str(opts)), (v.Grid(), v.Texels()), want)
        if path == "kept":                                              # (the first launch built the queue; its Sync read the lengths)
            v.Sync()
            launch(v, N, part)
            st = v.stats()
            self.differs(what + (path, str(opts), "second launch"), (v.Grid(), v.Texels()), want)
        self.launches += 1
        if proven(path, st, first):
            self.took.setdefault(path, set()).add(tag)
        return st

    def done(self):
        assert not self.bad, (len(self.bad), self.bad[:40])


# ---- 1: the lattice fuzz -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("path", ALL_PATHS)
def test_lattice_meshes_every_path(vox, orc, path):
    """Every lattice case at 16 and 32 through every setting of `path` (the lists' paths on the automatic, a coarse and a fine map), and
    the path proven on one case or more whose image depends on the winner of a tie."""
    run = Run(vox, orc)
    tied = set()
    for seed, n_tris, N, vb, ib, want, ties in lattice_cases(orc):
        if ties:
            tied.add((seed, N))
        for listres in ((0, 16, 512) if path in LIST_PATHS else (0,)):
            for opts, prep in settings_of(path, listres):
                run.compare((seed, n_tris, N), path, opts, prep, vb, ib, N, want, tag=(seed, N))
    run.done()
    assert run.took.get(path, set()) & tied, (path, sorted(run.took.get(path, ())), sorted(tied))


# ---- 2: needles --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("path", ("prepared", "queue", "box"))
def test_needles_and_slivers(vox, orc, path):
    """Needles aimed at the rays (footprints a fraction of a texel wide, edge functions that all but vanish) on a coarse, a medium and the
    finest map: the barycentrics of a sliver's hit are what the image is made of.  Brute force."""
    run = Run(vox, orc)
    rng = np.random.default_rng(2024)
    for n_tris, N in ((30, 16), (300, 32)):
        vb, ib = needle_mesh(rng, n_tris, N)
        want = orc.Scene(vb, ib).voxelize(N, algo=orc.ALGO_BRUTE, texels=True)
        assert want[0].sum() > 0 and np.array_equal(want[1] != 0, want[0] != 0)
        for listres in (16, 256, 4096):
            for opts, prep in settings_of(path, listres):
                st = run.compare((n_tris, N), path, opts, prep, vb, ib, N, want, tag=(n_tris, N, listres))
                assert st["list_entries"] > 0 and st["list_res"] == listres, (n_tris, N, listres, st["list_entries"], st["list_res"])
    run.done()
    assert len(run.took.get(path, ())) == 6, (path, run.took)             # every mesh on every map took the path


# ---- 3: the tie nobody sees --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("path", ALL_PATHS)
def test_doubled_sphere_ties_decide_the_image_only(vox, orc, path):
    """The sphere whose every triangle is there twice, the copy's normals turned (test_fuzz.doubled_sphere), at 64^3 in both index orders:
    the same grid either way and images that differ in most solid voxels (asserted on the oracle alone, its BVH: brute force takes
    seconds here) -- so a kernel that breaks the tie its own way passes every grid test there is and fails here."""
    N = 64
    if N not in _SPHERE:
        _SPHERE[N] = doubled_sphere_wanted(orc, N)
    vb2, orders, want = _SPHERE[N]
    run = Run(vox, orc)
    for first, ib2 in enumerate(orders):
        for opts, prep in settings_of(path):
            st = run.compare(("doubled sphere", first), path, opts, prep, vb2, ib2, N, want[first], tag=first)
            if path == "prepared":
                assert st["plan_prepared"] == 1 and st["list_entries"] > 0, (first, opts)
    run.done()
    assert run.took.get(path) == {0, 1}, (path, run.took)


# ---- 4: slabs and shares -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("path", ("prepared", "queue", "tree"))
def test_slabs_and_shares(vox, orc, path):
    """One lattice case (seed 9, 150 triangles, 32^3) as two slabs whose last brick layer is clamped and as rank 1 of 2 of a block-cyclic
    partition: the slices of the oracle's image the partition names, in its order."""
    (_, _, N, vb, ib, want, ties), = [c for c in lattice_cases(orc) if c[0] == 9 and c[2] == 32]
    assert ties
    run = Run(vox, orc)
    parts = (("slab", 3, 5), ("slab", 10, 1), ("share", 1, 2, 4))
    assert slices_of(N, parts[2]) == [z for z in range(N) if (z // 4) % 2 == 1]
    for part in parts:
        for opts, prep in settings_of(path):
            run.compare((9, 150, N, part), path, opts, prep, vb, ib, N, want, part=part, tag=part)
    run.done()
    assert run.took.get(path) == set(parts), (path, run.took)
