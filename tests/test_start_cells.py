"""The lists' start cells (dxv_dirmap.h: dm_start_cell, dm_start_cell_begin) on the CPU, through tests/hostcheck/start_cells_check.cpp.

A start cell is its texel's canonical cell with the start table's word where the search hints are; the body that reads it begins a scan
at the table's start (lists of up to kDmStartCellDirect entries) or at the later of a search over the whole list and the table's start.
For every texel and every probe radius of test_start_table.py -- and the half beyond r1max, a ray that is not live -- that start is never
behind the exact first entry with !(r1 < near); and grids and texel images through the new body equal those through the body of before
and those without a table."""
import ctypes as C

import numpy as np
import pytest

from start_table_cases import made_up_lists, stack, two_shells
from start_cells_cases import PROBE, HostCells, cells_library, check_start_cells


def check_probe(p, what):
    print(what, p)
    assert p["probes"] > 0 and p["late"] == 0 and p["not_live_wrong"] == 0, (what, p)


def check_host(h, what):
    cells, _ = h.lists()
    check_start_cells(h.start_cells, cells, h.starts)
    p = h.probe_cells()
    check_probe(p, what)
    return p


@pytest.mark.parametrize("name,R", [("bunny", 64), ("bunny", 256), ("dragon", 64), ("dragon", 256)])
def test_meshes_every_texel_every_probe(request, name, R):
    vb, ib, _ = request.getfixturevalue(name)
    h = HostCells(vb, ib, R)
    try:
        p = check_host(h, (name, R))
        assert p["moved"] > 0
    finally:
        h.close()


def same_grids(h, N, texels):
    """forms 1 (before), 2 (the table kernels), 3 (the brick box) against form 0 (no table)"""
    want = h.voxelize_form(N, 0, texels=texels)
    for form in (1, 2, 3):
        got = h.voxelize_form(N, form, texels=texels)
        if texels:
            assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), (N, form)
        else:
            assert np.array_equal(got, want), (N, form)
    return want


def test_two_shells_and_the_stack():
    h = HostCells(*two_shells(), 64)
    try:
        p = check_host(h, "two shells")
        assert p["moved"] > p["probes"] // 8
        assert same_grids(h, 32, False).any()
        g, t = same_grids(h, 32, True)
        assert g.any() and t.any()
    finally:
        h.close()
    h = HostCells(*stack(300), 16)
    try:
        p = check_host(h, "stack of 300")
        assert p["longest"] >= 300 and p["searched"] >= 1 and p["search_loads"] > 0      # the texel that counts in units of two, searched
        assert same_grids(h, 32, False).any()
        g, t = same_grids(h, 32, True)
        assert g.any() and t.any()
    finally:
        h.close()


def test_bunny_grids_and_texel_image(bunny):
    vb, ib, _ = bunny
    h = HostCells(vb, ib, 64)
    try:
        for N in (64, 50):
            assert same_grids(h, N, False).any(), N
            g, t = same_grids(h, N, True)
            assert g.any() and t.any(), N
    finally:
        h.close()


def test_made_up_lists():
    """the lists of test_start_table.py, and lists of exactly 35, 36 and kDmStartCellDirect, kDmStartCellDirect + 1 entries: the last that
    begins without a search and the first that searches, in one shell, in two, and with all far radii equal"""
    L = cells_library()
    T = int(L.sc_direct())
    rng = np.random.default_rng(7)
    lists = [[], [0x3800], [0x0400], [0x7bff]]
    lists += [sorted(rng.integers(0x3000, 0x3a00, n).tolist()) for n in (8, 9, 9, 17, 18, 35, 36)]
    lists += [[0x3456] * n for n in (1, 8, 9, 40, 300)]
    lists += [sorted([0x3400 + int(x) for x in rng.integers(0, 6, n // 2)] + [0x3900 + int(x) for x in rng.integers(0, 6, n - n // 2)]) for n in (9, 12, 17, 25, 35)]
    lists += [sorted(rng.integers(0x0400, 0x7c00, 64).tolist()), [0x0400, 0x7bff], [0x0400] * 5 + [0x7bff]]
    lists += [sorted(rng.integers(0x2000, 0x4000, n).tolist()) for n in (255, 256, 257, 511, 512, 513, 65535)]
    lists += [[0x3000] * 400 + [0x3800] * 200, [0x3000 + k // 3 for k in range(700)]]
    edge = sorted({35, 36, T, T + 1})
    lists += [sorted(rng.integers(0x3000, 0x3a00, n).tolist()) for n in edge]
    lists += [sorted([0x3400 + int(x) for x in rng.integers(0, 6, n // 2)] + [0x3900 + int(x) for x in rng.integers(0, 6, n - n // 2)]) for n in edge]
    lists += [[0x3456] * n for n in edge]
    cells, entries = made_up_lists(lists)
    starts = np.zeros(len(cells), np.uint32)
    out8 = np.zeros(8, np.uint64)
    L.st_probe_raw(cells.ctypes.data_as(C.c_void_p), len(cells), entries.ctypes.data_as(C.c_void_p), starts, out8.ctypes.data_as(C.c_void_p))
    start_cells = np.zeros_like(cells)
    L.sc_cells_raw(cells.ctypes.data_as(C.c_void_p), len(cells), entries.ctypes.data_as(C.c_void_p), start_cells.ctypes.data_as(C.c_void_p))
    check_start_cells(start_cells, cells, starts)
    for direct in sorted({T, 35, 64, 128, 0, 65535}):                   # (the replay's other thresholds; none; every list without a search)
        out = np.zeros(len(PROBE), np.uint64)
        L.sc_probe_raw(start_cells.ctypes.data_as(C.c_void_p), None, None, len(cells), entries.ctypes.data_as(C.c_void_p), direct, out.ctypes.data_as(C.c_void_p))
        p = dict(zip(PROBE, (int(x) for x in out)))
        check_probe(p, ("made-up lists", direct))
        assert p["texels"] == len(lists) - 1 and p["longest"] == 65535 and p["moved"] > 0
        assert p["searched"] == sum(1 for keys in lists if len(keys) > direct)
        assert (p["search_loads"] > 0) == (direct < 65535)
