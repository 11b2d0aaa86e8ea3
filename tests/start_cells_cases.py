"""The host library of tests/hostcheck/start_cells_check.cpp and a mesh's host-built lists with their start cells, shared by
tests/test_start_cells.py and tests/test_gpu_start_cells.py."""
import ctypes as C

import numpy as np

from start_table_cases import HostLists
from tools.round_stats import library

PROBE = ("probes", "late", "not_live_wrong", "texels", "searched", "longest", "moved", "first_bad", "search_loads", "earlier", "later")


def cells_library():
    return library(cells=True)


def word_of(start_cells):
    """the start word a start cell carries where the hints were: q1 | q2 << 16 (bytes 10 .. 13 of the cell)"""
    return (start_cells[:, 2] >> 16) | ((start_cells[:, 3] & 0xffff) << 16)


def check_start_cells(start_cells, cells, starts):
    """begin, count, r1max, thick byte for byte the canonical cell's; the table's word in q1, q2; q3 = 0"""
    assert start_cells.shape == cells.shape and start_cells.dtype == np.uint32
    assert np.array_equal(start_cells[:, :2], cells[:, :2])
    assert np.array_equal(start_cells[:, 2] & 0xffff, cells[:, 2] & 0xffff)
    assert np.array_equal(word_of(start_cells), starts)
    assert not (start_cells[:, 3] >> 16).any()


class HostCells(HostLists):
    """HostLists through the library that also holds the start cells' functions, with the lists' start cells"""

    def __init__(self, vb, ib, R):
        from oracle import orc
        self.L = cells_library()
        self.R = R
        vb, ib = np.ascontiguousarray(vb, np.float32), np.ascontiguousarray(ib, np.uint32)
        _, b = orc.bound(vb)
        self.h = self.L.hc_scene_create(vb, len(vb), ib, len(ib) // 3, b)
        self.n = self.L.hc_dirmap_build(self.h, R)
        self.starts = np.zeros(6 * R * R, np.uint32)
        self.L.st_table(self.h, self.starts)
        self.start_cells = np.zeros((6 * R * R, 4), np.uint32)
        self.L.sc_cells(self.h, self.start_cells.ctypes.data_as(C.c_void_p))

    def probe_cells(self, direct=None):
        out = np.zeros(len(PROBE), np.uint64)
        self.L.sc_probe(self.h, self.start_cells.ctypes.data_as(C.c_void_p), self.starts.ctypes.data_as(C.c_void_p),
                        int(self.L.sc_direct()) if direct is None else direct, out.ctypes.data_as(C.c_void_p))
        return dict(zip(PROBE, (int(x) for x in out)))

    def voxelize_form(self, N, form, texels=False):
        """form 0: no table; 1: canonical cell and the table's word (the body of before); 2: start cells (the table kernels' body);
        3: the brick-box body with start cells"""
        g = np.zeros((N, N, N), np.uint8)
        t = np.zeros((N, N, N), np.uint32) if texels else None
        rc = self.L.sc_voxelize(self.h, N, 1 if texels else 2, form, self.starts.ctypes.data_as(C.c_void_p) if form in (1, 3) else None,
                                self.start_cells.ctypes.data_as(C.c_void_p) if form in (2, 3) else None, g, t.ctypes.data_as(C.c_void_p) if texels else None)
        assert rc == 0
        return (g, t) if texels else g
