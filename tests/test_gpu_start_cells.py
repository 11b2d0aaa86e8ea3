"""The lists' start cells on the device: the array dirmap_starts makes beside the table equals the host's cell for cell while cells, entries and
table stay what they were; it is made again wherever the lists are -- a refit, an import into a context that held another scene, a smaller
mesh -- so that a grid through the kernels that read it equals the tree walk's; and option starttable switched 1 -> 0 -> 1 between the
launches of one context gives the same grid through every launch path."""
import ctypes as C

import numpy as np
import pytest

from dxrvoxelizer_amd.voxelizer import DBG_LIST_CELLS, DBG_LIST_ENTRIES, DBG_LIST_START_CELLS, DBG_LIST_STARTS
from start_table_cases import stack, two_shells
from start_cells_cases import HostCells, cells_library, check_start_cells
from test_gpu_start_table import every_path

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dxv(dxvlib):
    import dxrvoxelizer_amd
    return dxrvoxelizer_amd


@pytest.mark.parametrize("name,R", [("bunny", 64), ("stack", 16)])
def test_device_start_cells_equal_the_hosts(dxv, request, name, R):
    vb, ib = stack(300) if name == "stack" else request.getfixturevalue(name)[:2]
    h = HostCells(vb, ib, R)
    try:
        cells, entries = h.lists()
        check_start_cells(h.start_cells, cells, h.starts)
        for on in (1, 0):                                               # (made with the lists whatever the option says)
            v = dxv.Voxelizer(0)
            try:
                v.set_option("starttable", on)
                v.set_option("listres", R)
                v.InitFromArrays(vb, ib)
                v.set_option("lists", 2)
                v.Voxelize(32)
                st = v.stats()
                assert st["list_entries"] == h.n and st["list_res"] == R
                got = v.debug(DBG_LIST_START_CELLS)
                diff = np.flatnonzero((got != h.start_cells).any(axis=1))
                assert diff.size == 0, (on, diff[:8], got[diff[:8]], h.start_cells[diff[:8]])
                assert np.array_equal(v.debug(DBG_LIST_CELLS), cells) and np.array_equal(v.debug(DBG_LIST_ENTRIES), entries), on
                assert np.array_equal(v.debug(DBG_LIST_STARTS), h.starts), on
            finally:
                v.close()
        if name == "stack":
            assert (cells[:, 1] & 0xffff).max() > 255                    # the texel that counts in units of two
        assert np.count_nonzero(h.starts >> 4) > 0
    finally:
        h.close()


def current(v, N, what):
    """the context's start cells are those of the lists it holds NOW (the host's functions on the downloaded cells and entries), a grid
    through the kernels that read them equals the tree walk's, and the list check finds nothing"""
    v.set_option("starttable", 1)
    v.set_option("lists", 0)
    v.Voxelize(N)
    assert v.stats()["list_entries"] == 0, what
    want = v.Grid().copy()
    v.set_option("lists", 2)
    v.Voxelize(N)
    st = v.stats()
    assert st["list_entries"] > 0 and np.array_equal(v.Grid(), want) and want.any(), what
    cells, entries, starts, got = v.debug(DBG_LIST_CELLS), v.debug(DBG_LIST_ENTRIES), v.debug(DBG_LIST_STARTS), v.debug(DBG_LIST_START_CELLS)
    check_start_cells(got, cells, starts)
    host = np.zeros_like(cells)
    spare = np.concatenate([entries, np.zeros((4, 4), np.uint32)])
    cells_library().sc_cells_raw(cells.ctypes.data_as(C.c_void_p), len(cells), spare.ctypes.data_as(C.c_void_p), host.ctypes.data_as(C.c_void_p))
    assert np.array_equal(got, host), what
    accepted, violations, first = v.list_check(N)
    assert accepted > 0 and violations == 0, (what, violations, first)
    return st, got


def test_start_cells_follow_the_lists(dxv, bunny, dragon):
    import torch
    vb, ib, _ = bunny

    # squash the mesh and refit: the lists are built again, and the start cells with them
    v = dxv.Voxelizer(0)
    try:
        v.InitDynamic(vb, ib)
        _, before = current(v, 64, "before the refit")
        moved = np.array(vb, np.float32, copy=True)
        moved[:, 0] *= 0.5
        v.UpdateVertices(moved)
        _, after = current(v, 64, "refitted")
        assert before.shape != after.shape or not np.array_equal(before, after)
    finally:
        v.close()

    # export a blob, import it into a context that held another scene: the start cells are made there from the imported cells and entries
    dvb, dib, _ = dragon
    a, b = dxv.Voxelizer(0), dxv.Voxelizer(0)
    try:
        a.InitFromArrays(dvb, dib, gridDim=64)
        n = a.scene_bytes()
        blob = torch.empty(n, dtype=torch.uint8, device="cuda")
        a.scene_export(blob.data_ptr(), n)
        torch.cuda.synchronize()
        b.InitFromArrays(vb, ib, gridDim=64)
        b.set_option("starttable", 1)
        b.Voxelize(64)
        held = b.debug(DBG_LIST_START_CELLS)
        b.scene_import(blob.data_ptr(), n)
        st, got = current(b, 64, "imported")
        assert held.shape != got.shape or not np.array_equal(held, got)
        a.Voxelize(64)
        assert st["list_entries"] == a.stats()["list_entries"] and st["list_res"] == a.stats()["list_res"]
        assert np.array_equal(a.debug(DBG_LIST_START_CELLS), got)
    finally:
        a.close(), b.close()

    # InitFromArrays with a smaller mesh: the lists of the new mesh, the start cells of the new lists -- the host's
    v = dxv.Voxelizer(0)
    try:
        v.InitFromArrays(dvb, dib, gridDim=64)
        v.set_option("starttable", 1)
        v.Voxelize(64)
        svb, sib = two_shells()
        v.InitFromArrays(svb, sib, gridDim=64)
        st, got = current(v, 64, "a smaller mesh")
        h = HostCells(svb, sib, st["list_res"])
        try:
            assert st["list_entries"] == h.n and np.array_equal(got, h.start_cells)
        finally:
            h.close()
    finally:
        v.close()


@pytest.mark.parametrize("N", [64, 50])
def test_switching_the_table_between_launches(dxv, bunny, N):
    """1 -> 0 -> 1 in one context: the kernels that read the start cells, the plain ones, the first again -- every launch path, the same grid
    (N = 50 is no multiple of 16: the clear's fallback kernel)"""
    vb, ib, _ = bunny
    v = dxv.Voxelizer(0)
    try:
        v.InitFromArrays(vb, ib, gridDim=N)
        v.set_option("lists", 0)
        v.Voxelize(N)
        assert v.stats()["list_entries"] == 0
        want = v.Grid().copy()
        assert want.any()
        v.set_option("lists", 2)
        for on in (1, 0, 1):
            v.set_option("starttable", on)
            every_path(v, N, want, None, ("bunny", N, "starttable", on))
        assert v.list_check(N)[1] == 0
    finally:
        v.close()
