"""The product's octree routines on the CPU: tests/hostcheck/octree_check.cpp (which includes csrc/dxv_octree.h) compiled into a small
library of its own, the way tests/isosurface_host.py compiles the isosurface routines."""
import ctypes as C
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_LIB = None
_U8 = np.ctypeslib.ndpointer(np.uint8, flags="C")
_U32 = np.ctypeslib.ndpointer(np.uint32, flags="C")
EMPTY, FULL, MIXED, BAD = 0, 1, 2, 3                                   # OCT_* of csrc/dxv_octree.h


def library():
    global _LIB
    if _LIB is None:
        src = os.path.join(ROOT, "tests", "hostcheck", "octree_check.cpp")
        so = os.path.join(ROOT, "tests", "hostcheck", "liboctreecheck.so")
        deps = [src] + [os.path.join(ROOT, "dxrvoxelizer_amd", "csrc", h) for h in ("dxv_octree.h", "dxv_types.h")]
        if not os.path.exists(so) or os.path.getmtime(so) < max(os.path.getmtime(d) for d in deps):
            subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-Wall", "-Werror",
                                   "-Wno-unknown-pragmas", "-o", so, src])
        L = C.CDLL(so)
        L.oc_build.argtypes = [_U8, C.c_uint32, C.c_void_p, C.c_void_p]
        L.oc_build.restype = C.c_int
        L.oc_expand.argtypes = [_U32, C.c_uint32, C.c_uint32, C.c_uint32, _U8]
        L.oc_expand.restype = C.c_uint64
        L.oc_lookup_guarded.argtypes = [_U32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32]
        L.oc_lookup_guarded.restype = C.c_int
        _LIB = L
    return _LIB


def build(grid):
    """(nodes [n, 2] uint32, level_first) of a uint8 [N, N, N] grid by the product's own routines, in the kernels' order"""
    grid = np.ascontiguousarray(grid, np.uint8)
    N = grid.shape[0]
    assert grid.shape == (N, N, N)
    out = np.zeros(14, np.uint64)
    assert library().oc_build(grid, N, out.ctypes.data_as(C.c_void_p), None) == 0
    nodes = np.empty((int(out[1]), 2), np.uint32)
    assert library().oc_build(grid, N, out.ctypes.data_as(C.c_void_p), nodes.ctypes.data_as(C.c_void_p)) == 0
    return nodes, [int(v) for v in out[2:3 + int(out[0])]]


def expand(nodes, levels, N):
    """(grid [N, N, N] of 0 / 1, voxels refused) by oct_lookup for every voxel"""
    nodes = np.ascontiguousarray(nodes, np.uint32).reshape(-1, 2)
    grid = np.empty((N, N, N), np.uint8)
    refused = library().oc_expand(nodes, len(nodes), int(levels), N, grid)
    return grid, int(refused)


def lookup_guarded(nodes, levels, x, y, z):
    """oct_lookup of one voxel on a copy of the tree with an inaccessible page right behind its last node"""
    nodes = np.ascontiguousarray(nodes, np.uint32).reshape(-1, 2)
    return library().oc_lookup_guarded(nodes, len(nodes), int(levels), x, y, z)
