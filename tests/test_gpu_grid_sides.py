"""Every even side from 2 to 72, and three longer rows, through every operator of a frame's grid on the GPU (tests/grid_sides.py: the sides,
the grids and why these).  The headers' routines are run at the same sides on the CPU by the *_rule tests; what exists only in the .hip files
-- the kernels' own indexing, the choice between the 8-byte and the guarded byte path, the launch geometry, the ballot packing -- runs here.
Each grid is written through the frame's grid pointer and every result is compared with the numpy restatement of the same operation by
array_equal: no tolerance, no side, grid or operator skipped.  After each operator that edits the grid the whole grid is read back, so a
guarded path that spills into the next row shows.  One more test per side launches the bunny and the cube in the four modes, prepared,
unprepared and through the tree, and compares the mesh distance field.  At the longer rows distance and components are compared with scipy,
which the restatements are checked against on the CPU."""
import numpy as np
import pytest

import components_restated as cr
import distance_restated as dr
import fill_restated as fr
import grid_sides as gs
import morph_restated as mr
import octree_restated as orr
import surface_restated as sr
import test_gpu_components as tgc
import test_gpu_isosurface as tgi
import test_gpu_mesh_distance as tgm
import test_gpu_octree as tgo
from raycast_restated import write_grid
from test_gpu_distance import check_field
from test_gpu_fill import check_fill
from test_gpu_morph import check_morph
from test_gpu_prepared import poison

try:
    from scipy import ndimage
except ImportError:                                                     # without scipy the longer rows go through the numpy restatements: minutes, not seconds
    ndimage = None

pytestmark = pytest.mark.gpu

MORPH_RADII = (1, 10)
OTHER_PAIRS = [N for N in gs.SWEEP if N % 8 in (2, 6) or N in (4, 64, 72)]      # the sides that also label (SOLID, 26) and (EMPTY, 6)
ISO_SIDES = gs.SWEEP                    # one extraction of the restatement stays under half a second up to 72 (profiles/NOTES.md): no side is left out
BUNNY_WHOLE_UP_TO, BUNNY_UP_TO = 8, 32  # the mesh distance restatement tries every triangle at every voxel: the bunny's 69 666 cost 4 s at 8^3 and 46 s at 16^3,
                                        # so from 10 to 32 the bunny is thinned to every 70th triangle (996: 5 s at 32^3); the cube runs at every side
POISON = 0xAA


@pytest.fixture(scope="module")
def dxv(dxvlib):
    import dxrvoxelizer_amd
    return dxrvoxelizer_amd


@pytest.fixture(scope="module")
def writer(dxv, bunny):
    """the one Voxelizer, on the bunny, whose frame every grid of this file is written into"""
    vb, ib, _ = bunny
    v = dxv.Voxelizer(0)
    v.InitFromArrays(vb, ib)
    yield v
    v.close()


def random_grid(name):
    return name.startswith("random")


def has_both_kinds(g):
    return bool((g != 0).any() and (g == 0).any())


def names_at(N):
    """the grids of a side: the sweep's five (four below 6), three of them at the longer rows"""
    return gs.WIDE_GRIDS if N in gs.WIDE else None


# ---- count, bits, fill -------------------------------------------------------------------------------------------------------------------
def check_count_and_bits(v, g, what):
    assert v.CountSolid() == int(np.count_nonzero(g)), what
    assert np.array_equal(v.GridBits(), np.packbits(g.reshape(-1) != 0, bitorder="little")), what
    assert np.array_equal(v.Grid(), g), what


def check_fill_both_batches(v, g, what):
    """both kinds with the default rounds per batch and with one, the settle path; returns the outside set"""
    try:
        for batch in (0, 1):
            v.set_option("fillrounds", batch)
            out = check_fill(v, g, lambda: write_grid(v, g), f"{what}, fillrounds {batch}")
    finally:
        v.set_option("fillrounds", 0)
    return out


@pytest.mark.parametrize("N", gs.SWEEP + gs.WIDE)
def test_count_bits_and_fill(writer, N):
    v = writer
    v.Voxelize(N)
    for name, g in gs.grids(N, names_at(N)):
        what = f"N = {N}, {name}"
        write_grid(v, g)
        check_count_and_bits(v, g, what)
        out = check_fill_both_batches(v, g, what)
        if random_grid(name) and N >= 8:
            assert has_both_kinds(g), what
        if name == "hollow box":
            assert int(np.count_nonzero(~out & (g == 0))) == (N - 4) ** 3 > 0, what       # the fill changes the box's inside: no empty comparison


# ---- distance ------------------------------------------------------------------------------------------------------------------------------
def scipy_distance_sq(g):
    """the exact squared distances by scipy's Euclidean transform, in the field's convention; exact in float64 at these sides"""
    s = g != 0
    if s.all() or not s.any():
        return np.full(g.shape, -dr.NONE if s.all() else dr.NONE, np.int32)
    return np.where(s, -np.rint(ndimage.distance_transform_edt(s) ** 2), np.rint(ndimage.distance_transform_edt(~s) ** 2)).astype(np.int32)


@pytest.mark.parametrize("N", gs.SWEEP)
def test_distance_field_in_both_formats(dxv, writer, N):
    v = writer
    v.Voxelize(N)
    for name, g in gs.grids(N):
        write_grid(v, g)
        grid, _ = check_field(v, dxv, f"N = {N}, {name}")
        assert np.array_equal(grid, g)


@pytest.mark.parametrize("N", gs.WIDE)
def test_distance_field_of_longer_rows(dxv, writer, N):
    v = writer
    v.Voxelize(N)
    for name, g in gs.grids(N, gs.WIDE_GRIDS):
        write_grid(v, g)
        want = scipy_distance_sq(g) if ndimage else dr.distance_sq(g)
        got = v.DistanceField(dxv.DIST_SQ_I32)
        assert got.dtype == np.int32 and np.array_equal(got, want), (N, name)
        assert np.array_equal(v.Grid(), g), (N, name)


# ---- components ----------------------------------------------------------------------------------------------------------------------------
def check_components(v, N, name, g, pairs):
    """the labelling of each (kind, connectivity) of `pairs` against the restatement; {pair: K}"""
    key = f"sides {name} {N}"
    counts = {}
    try:
        for of, conn in pairs:
            write_grid(v, g)
            _, table = tgc.check(v, key, g, of, conn)
            counts[of, conn] = len(table)
        assert np.array_equal(v.Grid(), g), key                         # labelling edits nothing
    finally:
        for k in [k for k in tgc._RESTATED if k[0] == key]:             # (this side's restatements are not needed again)
            del tgc._RESTATED[k]
    return counts


@pytest.mark.parametrize("N", gs.SWEEP)
def test_components_solid_6_and_empty_26(writer, N):
    v = writer
    v.Voxelize(N)
    for name, g in gs.grids(N):
        counts = check_components(v, N, name, g, ((cr.SOLID, 6), (cr.EMPTY, 26)))
        if random_grid(name) and N >= 8:
            assert counts[cr.SOLID, 6] > 1, (N, name)


@pytest.mark.parametrize("N", OTHER_PAIRS)
def test_components_solid_26_and_empty_6(writer, N):
    v = writer
    v.Voxelize(N)
    for name, g in gs.grids(N):
        check_components(v, N, name, g, ((cr.SOLID, 26), (cr.EMPTY, 6)))


@pytest.mark.parametrize("N", gs.SWEEP)
def test_select_components_on_the_random_grid(writer, N):
    v = writer
    v.Voxelize(N)
    key = f"sides select {N}"
    try:
        tgc.check_select(v, key, gs.random_grid(N, 0.6))
    finally:
        for k in [k for k in tgc._RESTATED if k[0] == key]:
            del tgc._RESTATED[k]


def scipy_label(g, of, conn):
    """(labels, table) as components_restated.label gives them, from scipy's labelling numbered again by first voxel"""
    m = cr.members(g, of)
    N = m.shape[0]
    lab, K = ndimage.label(m, structure=ndimage.generate_binary_structure(3, 1 if conn == 6 else 3))
    values, where = np.unique(lab.ravel(), return_index=True)
    values, where = values[values > 0], where[values > 0]
    rank = np.zeros(K + 1, np.uint32)
    rank[values[np.argsort(where, kind="stable")]] = np.arange(1, K + 1, dtype=np.uint32)
    labels = rank[lab]
    table = np.zeros(K, cr.RECORD)
    if K:
        z, y, x = np.nonzero(m)
        k = labels[m].astype(np.int64) - 1
        table["first"] = np.sort(where)
        table["voxels"] = np.bincount(k, minlength=K)
        order = np.argsort(k, kind="stable")
        starts = np.searchsorted(k[order], np.arange(K))
        for axis, c in enumerate((x, y, z)):
            table["lo"][:, axis] = np.minimum.reduceat(c[order], starts)
            table["hi"][:, axis] = np.maximum.reduceat(c[order], starts)
        border = (x == 0) | (x == N - 1) | (y == 0) | (y == N - 1) | (z == 0) | (z == N - 1)
        table["flags"] = (np.bincount(k, weights=border, minlength=K) > 0).astype(np.uint32)
    return labels, table


@pytest.mark.parametrize("N", gs.WIDE)
def test_components_of_longer_rows(writer, N):
    v = writer
    v.Voxelize(N)
    for name, g in gs.grids(N, gs.WIDE_GRIDS):
        for of, conn in ((cr.SOLID, 6), (cr.EMPTY, 26)):
            write_grid(v, g)
            want, wtable = scipy_label(g, of, conn) if ndimage else cr.label(g, of, conn)
            labels, table = v.Components(of, conn)
            assert labels.dtype == np.uint32 and np.array_equal(labels, want), (N, name, of, conn)
            assert table.dtype == cr.RECORD and np.array_equal(table, wtable), (N, name, of, conn)
            assert v.components_info() == (len(wtable), of, conn), (N, name)
            if random_grid(name) and of == cr.SOLID:
                assert len(wtable) > 1, (N, name)
        assert np.array_equal(v.Grid(), g), (N, name)


# ---- morph ---------------------------------------------------------------------------------------------------------------------------------
def check_morph_both_forms(v, g, ops, radii, what):
    """every (operation, radius) through the bit planes and through the field form; {(op, r2): (set, cleared)}"""
    changed = {}
    try:
        for r2 in radii:
            for op in ops:
                want = mr.morph(g, op, r2)
                changed[op, r2] = mr.counts(g, want)
                for form in (1, 2):
                    v.set_option("morphform", form)
                    check_morph(v, g, lambda: write_grid(v, g), op, r2, want, f"{what}, form {form}")
    finally:
        v.set_option("morphform", 0)
    return changed


@pytest.mark.parametrize("N", gs.SWEEP)
def test_morph_in_both_forms(writer, N):
    v = writer
    v.Voxelize(N)
    for name, g in gs.grids(N):
        changed = check_morph_both_forms(v, g, mr.OPS, MORPH_RADII, f"N = {N}, {name}")
        if random_grid(name) and N >= 8:
            for r2 in MORPH_RADII:
                assert changed[mr.DILATE, r2][0] >= 1 and changed[mr.ERODE, r2][1] >= 1, (N, name, r2)


@pytest.mark.parametrize("N", gs.WIDE)
def test_dilate_and_erode_of_longer_rows(writer, N):
    v = writer
    v.Voxelize(N)
    for name, g in gs.grids(N, gs.WIDE_GRIDS):
        changed = check_morph_both_forms(v, g, (mr.DILATE, mr.ERODE), (10,), f"N = {N}, {name}")
        if random_grid(name):
            assert changed[mr.DILATE, 10][0] >= 1 and changed[mr.ERODE, 10][1] >= 1, (N, name)


# ---- octree and expansion ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", gs.SWEEP + gs.WIDE)
def test_octree_and_expansion(writer, N):
    v = writer
    v.Voxelize(N)
    for name, g in gs.grids(N, names_at(N)):
        what = f"N = {N}, {name}"
        write_grid(v, g)
        nodes = tgo.check(v, g, what)
        assert len(nodes) >= 1
        assert np.array_equal(v.Grid(), g), what                        # the build edits nothing
        write_grid(v, np.full((N, N, N), POISON, np.uint8))             # poison: every voxel must be written
        v.OctreeExpand()
        assert np.array_equal(v.Grid(), (g != 0).astype(np.uint8)), what


# ---- isosurface ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", ISO_SIDES)
def test_isosurface_of_the_grid_distance_field(dxv, writer, N):
    v = writer
    v.Voxelize(N)
    for name, g in gs.grids(N):
        write_grid(v, g)
        v.DistanceField(dxv.DIST_F32)
        n = tgi.all_levels_and_spaces(v, dxv, dxv.ISO_GRID_DISTANCE, tgi.F32(1.0), f"N = {N}, {name}")
        assert n > 0, (N, name)                                         # every grid of the sweep has solid voxels


# ---- the launches -----------------------------------------------------------------------------------------------------------------------------
def launch_all_modes(v, dxv, N, want, want_image, what, prepared=None):
    """every mode over a poisoned grid; the reference launch with the texel image on (it exists in that mode only), compared as well: the image
    the frame held before is the other mesh's or another way's, at the same side"""
    v.Voxelize(N)                                                       # (the frame's grid exists from the first launch on)
    for mode in (dxv.MODE_REFERENCE, dxv.MODE_PARITY, dxv.MODE_SURFACE, dxv.MODE_REFERENCE_SURFACE):
        poison(v, POISON)                                               # every voxel is written in every launch
        v.EnableTexels(mode == dxv.MODE_REFERENCE)
        try:
            v.Voxelize(N, mode)
            got = v.Grid()
            assert got.shape == want[mode].shape and np.array_equal(got, want[mode]), f"{what}, mode {mode}: {int((got != want[mode]).sum())} voxels differ"
            if mode == dxv.MODE_REFERENCE:
                image = v.Texels()
                assert image.shape == want_image.shape and np.array_equal(image, want_image), f"{what}: {int((image != want_image).sum())} texels differ"
        finally:
            v.EnableTexels(False)
        if prepared is not None and mode == dxv.MODE_REFERENCE:
            assert v.stats()["plan_prepared"] == prepared, (what, v.stats()["list_entries"])


@pytest.mark.parametrize("N", gs.SWEEP)
def test_launches_in_every_mode_three_ways(dxv, orc, bunny, N):
    from dxrvoxelizer_amd import meshes
    v, w = dxv.Voxelizer(0), dxv.Voxelizer(0)                           # (one pair for both meshes: the cube's launches find the bunny's texel image in the frame)
    try:
        w.set_option("lists", 0)                                        # w: every ray walks the tree
        for name, (vb, ib) in (("bunny", bunny[:2]), ("cube", meshes.cube())):
            scene = orc.Scene(vb, ib)
            (solid, image), surface = scene.voxelize(N, mode=orc.MODE_REFERENCE, texels=True), sr.surface_of_mesh(vb, ib, N)
            want = {dxv.MODE_REFERENCE: solid, dxv.MODE_PARITY: scene.voxelize(N, mode=orc.MODE_PARITY), dxv.MODE_SURFACE: surface,
                    dxv.MODE_REFERENCE_SURFACE: solid | surface}
            assert solid.any(), (name, N)
            assert np.array_equal(image != 0, solid != 0), (name, N)
            assert surface.any() or name == "cube", (name, N)         # (the cube's faces lie on the grid's outer voxel faces: at some sides float32 puts them outside, and the rule's surface is empty)
            v.InitFromArrays(vb, ib, gridDim=N)                         # Init with the grid hint: the launches run the prepared queue ...
            launch_all_modes(v, dxv, N, want, image, f"{name} {N} prepared", prepared=1 if name == "bunny" and N >= 34 else None)
            v.InitFromArrays(vb, ib)                                    # ... without it they build their own ...
            launch_all_modes(v, dxv, N, want, image, f"{name} {N} unprepared", prepared=0)
            w.InitFromArrays(vb, ib)                                    # ... and without lists every ray walks the tree
            launch_all_modes(w, dxv, N, want, image, f"{name} {N} tree walk", prepared=0)
            assert w.stats()["list_entries"] == 0
    finally:
        v.close()
        w.close()


# ---- the mesh distance field ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", gs.SWEEP)
def test_mesh_distance_field_with_triangles(dxv, bunny, N):
    from dxrvoxelizer_amd import meshes
    cases = [("cube", meshes.cube())]
    if N <= BUNNY_UP_TO:
        vb, ib, _ = bunny
        if N > BUNNY_WHOLE_UP_TO:
            ib = np.ascontiguousarray(ib.reshape(-1, 3)[::70].reshape(-1))
        cases.append((f"bunny, {len(ib) // 3} triangles", (vb, ib)))
    for name, (vb, ib) in cases:
        v = dxv.Voxelizer(0)
        try:
            v.InitFromArrays(vb, ib)
            v.Voxelize(N)
            _, _, tri = tgm.check(v, dxv, sr.normalised_tris(vb, ib), N, f"{name} {N}")
            assert (tri != tgm.NO).all()
        finally:
            v.close()
