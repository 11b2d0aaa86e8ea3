"""The lists' start table on the device: the table dirmap_starts makes equals the host's word for word, cells and entries are what they
were, grids (and the texel image) with option starttable 1 = 0 = the tree walk through every launch path, and the table follows the
lists through a refit, an import and another mesh -- with the extended list check (every accepted pair at or behind the table's start)
reporting no violation after each."""
import numpy as np
import pytest

from dxrvoxelizer_amd.slabs import interleaved_slices
from dxrvoxelizer_amd.voxelizer import DBG_LIST_CELLS, DBG_LIST_ENTRIES, DBG_LIST_STARTS
from start_table_cases import HostLists, stack, two_shells

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dxv(dxvlib):
    import dxrvoxelizer_amd
    return dxrvoxelizer_amd


def mesh_of(request, name):
    if name == "two_shells":
        return two_shells()
    if name == "stack":
        return stack(300)
    vb, ib, _ = request.getfixturevalue(name)
    return vb, ib


@pytest.mark.parametrize("name,R", [("bunny", 64), ("bunny", 256), ("turingbowl", 256), ("stack", 16)])
def test_device_table_equals_host_table(dxv, request, name, R):
    vb, ib = mesh_of(request, name)
    h = HostLists(vb, ib, R)
    got = {}
    try:
        for on in (1, 0):
            v = dxv.Voxelizer(0)
            try:
                v.set_option("starttable", on)
                v.set_option("listres", R)
                v.InitFromArrays(vb, ib)
                v.set_option("lists", 2)
                v.Voxelize(32)
                st = v.stats()
                assert st["list_entries"] == h.n and st["list_res"] == R
                got[on] = (v.debug(DBG_LIST_CELLS), v.debug(DBG_LIST_ENTRIES), v.debug(DBG_LIST_STARTS))
            finally:
                v.close()
        cells, entries = h.lists()
        for on in (1, 0):                                               # (the table is made with the lists whatever the option says)
            assert np.array_equal(got[on][0], cells) and np.array_equal(got[on][1], entries), on
            diff = np.flatnonzero(got[on][2] != h.starts)
            assert diff.size == 0, (on, diff[:8], got[on][2][diff[:8]], h.starts[diff[:8]])
        if name == "stack":
            assert (cells[:, 1] & 0xffff).max() > 255                    # the texel that counts in units of two
        assert np.count_nonzero(h.starts >> 4) > 0
    finally:
        h.close()


def every_path(v, N, want, want_texels, what):
    """the grid (and the texel image, when it is on) of every launch path against the tree walk's"""
    world, block = (4, 4) if N % 16 == 0 else (5, 2)

    def same(sel, path):
        g = v.Grid()
        assert g.shape == want[sel].shape and np.array_equal(g, want[sel]), (what, path, int((g != want[sel]).sum()))
        if want_texels is not None:
            assert np.array_equal(v.Texels(), want_texels[sel]), (what, path, "texels")
        assert v.stats()["list_entries"] > 0, (what, path)

    whole = slice(None)
    v.set_option("prepared", 1); v.set_option("plan", 2)
    v.PrepareLaunch(N)
    v.Voxelize(N)
    same(whole, "prepared")
    if N % 16 == 0:
        assert v.stats()["plan_prepared"] == 1, what
    v.set_option("prepared", 0)
    v.Voxelize(N)
    same(whole, "unprepared queue")
    assert v.stats()["plan_prepared"] == 0 and v.stats()["plan_bricks"] > 0
    v.set_option("plan", 1)
    v.Voxelize(N); v.Voxelize(N)
    same(whole, "kept queue")
    v.set_option("plan", 0)
    v.Voxelize(N)
    same(whole, "brick box")
    v.set_option("plan", 2)
    v.Voxelize(N, 0, N // 4, N // 2)
    same(slice(N // 4, N // 4 + N // 2), "slab")
    v.set_option("prepared", 1)
    v.PrepareLaunchInterleaved(N, 1, world, block)
    v.VoxelizeInterleaved(N, 1, world, block)
    same(interleaved_slices(N, 1, world, block), "interleaved share")


@pytest.mark.parametrize("name,N,R", [("bunny", 64, 0), ("bunny", 50, 0), ("two_shells", 32, 0), ("stack", 32, 16)])
def test_grids_with_the_table_without_it_and_the_tree_walk(dxv, request, name, N, R):
    vb, ib = mesh_of(request, name)
    v = dxv.Voxelizer(0)
    try:
        v.set_option("listres", R)
        v.InitFromArrays(vb, ib, gridDim=N)
        v.set_option("lists", 0)
        v.EnableTexels(True)
        v.Voxelize(N)
        assert v.stats()["list_entries"] == 0
        want, want_texels = v.Grid().copy(), v.Texels().copy()
        assert want.any()
        v.set_option("lists", 2)
        for texels in (False, True):
            v.EnableTexels(texels)
            for on in (1, 0, 2):
                v.set_option("starttable", on)
                every_path(v, N, want, want_texels if texels else None, (name, N, "starttable", on, "texels", texels))
        assert v.list_check(N)[1] == 0
    finally:
        v.close()


def test_the_table_follows_the_lists(dxv, bunny, dragon):
    import torch
    vb, ib, _ = bunny

    def against_the_tree_walk(v, N, what):
        v.set_option("lists", 0)
        v.Voxelize(N)
        assert v.stats()["list_entries"] == 0, what
        want = v.Grid().copy()
        v.set_option("lists", 2)
        v.Voxelize(N)
        st = v.stats()
        assert st["list_entries"] > 0 and np.array_equal(v.Grid(), want) and want.any(), what
        accepted, violations, first = v.list_check(N)
        assert accepted > 0 and violations == 0, (what, violations, first)
        return st

    # squash the mesh and refit: the lists are built again, and the table with them
    v = dxv.Voxelizer(0)
    try:
        v.InitDynamic(vb, ib)
        against_the_tree_walk(v, 64, "before the refit")
        before = v.debug(DBG_LIST_STARTS)
        moved = np.array(vb, np.float32, copy=True)
        moved[:, 0] *= 0.5
        v.UpdateVertices(moved)
        against_the_tree_walk(v, 64, "refitted")
        after = v.debug(DBG_LIST_STARTS)
        assert before.shape != after.shape or not np.array_equal(before, after)
    finally:
        v.close()

    # export a blob, import it into a second context: the table is made there from the imported cells and entries
    dvb, dib, _ = dragon
    a, b = dxv.Voxelizer(0), dxv.Voxelizer(0)
    try:
        a.InitFromArrays(dvb, dib, gridDim=64)
        n = a.scene_bytes()
        blob = torch.empty(n, dtype=torch.uint8, device="cuda")
        a.scene_export(blob.data_ptr(), n)
        torch.cuda.synchronize()
        b.InitFromArrays(vb, ib, gridDim=64)                            # (b held another scene's lists and table)
        b.Voxelize(64)
        b.scene_import(blob.data_ptr(), n)
        st = against_the_tree_walk(b, 64, "imported")
        a.Voxelize(64)
        assert st["list_entries"] == a.stats()["list_entries"] and st["list_res"] == a.stats()["list_res"]
        assert np.array_equal(a.debug(DBG_LIST_STARTS), b.debug(DBG_LIST_STARTS))
        assert np.array_equal(a.debug(DBG_LIST_CELLS), b.debug(DBG_LIST_CELLS))
    finally:
        a.close(), b.close()

    # set_mesh to a smaller mesh: the lists of the new mesh, the table of the new lists
    v = dxv.Voxelizer(0)
    try:
        v.InitFromArrays(dvb, dib, gridDim=64)
        v.Voxelize(64)
        svb, sib = two_shells()
        v.InitFromArrays(svb, sib, gridDim=64)
        st = against_the_tree_walk(v, 64, "a smaller mesh")
        h = HostLists(svb, sib, st["list_res"])
        try:
            assert st["list_entries"] == h.n and np.array_equal(v.debug(DBG_LIST_STARTS), h.starts)
        finally:
            h.close()
    finally:
        v.close()
