"""Meshes, made-up lists and the host library shared by tests/test_start_table.py and tests/test_gpu_start_table.py."""
import ctypes as C
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from tools.round_stats import library  # noqa: E402  (builds tests/hostcheck/libstartcheck.so when it is older than its sources)

_PINS = np.array([[-1, -1, -1, 0, 0, 1], [1, 1, 1, 0, 0, 1]], np.float32)     # unreferenced vertices: the bound is the cube [-1, 1]^3


def two_shells():
    """a small torus around the grid centre: every direction near its plane meets the tube twice -- a near and a far shell per texel"""
    from dxrvoxelizer_amd import meshes
    vb, ib = meshes.torus(48, 24, 0.6, 0.3)
    return np.concatenate([vb, _PINS]).astype(np.float32), ib


def stack(n=300):
    """n thin triangles behind one another over ONE direction (1, 0.06, 0.06), each well inside texel (8, 8) of a 16-texel face: that texel
    lists them all -- more than 255 entries, so the table counts in units of two -- and a 32^3 grid has voxels that look at them"""
    d = np.array([1.0, 0.06, 0.06])
    e1, e2 = np.array([0.0, 1.0, 0.0]), np.array([0.0, 0.0, 1.0])
    pos = []
    for k in range(n):
        x = 0.25 + 0.7 * k / n
        c, h = d * x, 0.04 * x
        pos += [c - h * e1 - h * e2, c + h * e1 - h * e2, c + h * e2]
    pos = np.array(pos, np.float32)
    vb = np.hstack([pos, np.tile(np.array([[1, 0, 0]], np.float32), (len(pos), 1))])
    return np.concatenate([vb, _PINS]).astype(np.float32), np.arange(3 * n, dtype=np.uint32)


class HostLists:
    """a mesh's lists built on the host with the product's footprint code, and their start table"""

    def __init__(self, vb, ib, R):
        from oracle import orc
        self.L = library()
        self.R = R
        vb, ib = np.ascontiguousarray(vb, np.float32), np.ascontiguousarray(ib, np.uint32)
        _, b = orc.bound(vb)
        self.h = self.L.hc_scene_create(vb, len(vb), ib, len(ib) // 3, b)
        self.n = self.L.hc_dirmap_build(self.h, R)
        self.starts = np.zeros(6 * R * R, np.uint32)
        self.L.st_table(self.h, self.starts)

    def lists(self):
        cells, entries = np.empty((6 * self.R * self.R, 4), np.uint32), np.empty((self.n, 4), np.uint32)
        self.L.hc_dirmap_get(self.h, cells.ctypes.data_as(C.c_void_p), entries.ctypes.data_as(C.c_void_p))
        return cells, entries

    def probe(self, starts=None):
        out = np.zeros(8, np.uint64)
        self.L.st_probe(self.h, self.starts if starts is None else starts, out.ctypes.data_as(C.c_void_p))
        return dict(zip(("probes", "late", "early", "texels", "over_255", "longest", "moved", "first_bad"), (int(x) for x in out)))

    def voxelize(self, N, table, texels=False):
        g = np.zeros((N, N, N), np.uint8)
        t = np.zeros((N, N, N), np.uint32) if texels else None
        rc = self.L.st_voxelize(self.h, N, 1 if texels else 2, self.starts.ctypes.data_as(C.c_void_p) if table else None, g,
                                t.ctypes.data_as(C.c_void_p) if texels else None)
        assert rc == 0
        return (g, t) if texels else g

    def close(self):
        if self.h:
            self.L.hc_scene_destroy(self.h)
            self.h = None


def made_up_lists(key_lists):
    """cells and entries (as the device holds them) of texels whose entries have the far-radius keys given, ascending: what the table
    reads of a list is its length, its keys and the cell's r1max"""
    cells, entries = [], []
    for keys in key_lists:
        begin = len(entries)
        for k in keys:
            r0 = max(k - 3, 1)
            entries.append([0, 0, ((0x7fff - r0) | (k << 16)) | 0x80008000, len(entries)])
        top = keys[-1] if keys else 0
        cells.append([begin, len(keys) | (top << 16), 0, 0])
    return np.array(cells, np.uint32).reshape(-1, 4), np.array(entries + [[0, 0, 0, 0]] * 4, np.uint32).reshape(-1, 4)
