"""The product's skeleton routines on the CPU: tests/hostcheck/skeleton_check.cpp (which includes csrc/dxv_skeleton.h and, through it,
csrc/dxv_components.h's union-find) compiled into a small library of its own, the way tests/access_host.py compiles the access's."""
import ctypes as C
import os
import subprocess

import numpy as np

import skeleton_restated as sr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADERS = ("dxv_skeleton.h", "dxv_components.h", "dxv_fill.h", "dxv_solid.h", "dxv_types.h")
_LIB = None


def library():
    global _LIB
    if _LIB is None:
        src = os.path.join(ROOT, "tests", "hostcheck", "skeleton_check.cpp")
        so = os.path.join(ROOT, "tests", "hostcheck", "libskeletoncheck.so")
        deps = [src] + [os.path.join(ROOT, "dxrvoxelizer_amd", "csrc", h) for h in HEADERS]
        if not os.path.exists(so) or os.path.getmtime(so) < max(os.path.getmtime(d) for d in deps):
            subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-Wall", "-Werror", "-Wno-unknown-pragmas", "-o", so, src])
        L = C.CDLL(so)
        u8 = np.ctypeslib.ndpointer(np.uint8, flags="C")
        L.sk_skeleton.argtypes = [u8, C.c_uint32, C.c_void_p, np.ctypeslib.ndpointer(np.uint64, flags="C")]
        L.sk_skeleton.restype = C.c_int
        L.sk_copy.argtypes = [np.ctypeslib.ndpointer(np.uint32, flags="C"), C.c_void_p, C.c_void_p]
        L.sk_copy.restype = None
        L.sk_prune.argtypes = [u8, C.c_uint32, C.c_uint32, np.ctypeslib.ndpointer(np.uint64, flags="C")]
        L.sk_prune.restype = C.c_int
        L.sk_valid.argtypes = [C.c_uint32]
        L.sk_max_n.restype = C.c_uint32
        _LIB = L
    return _LIB


def skeleton(grid, weights=None):
    """(labels uint32 [N, N, N], nodes [K], branches [B], (end, curve, junction voxels)) by the product's own routines, run serially"""
    g = np.ascontiguousarray(grid, np.uint8)
    N = g.shape[0]
    assert g.shape == (N, N, N)
    w = None if weights is None else np.ascontiguousarray(weights, np.uint32).reshape(-1)
    counts = np.zeros(5, np.uint64)
    rc = library().sk_skeleton(g, N, None if w is None else w.ctypes.data_as(C.c_void_p), counts)
    assert rc == 0, rc
    labels, nodes, branches = np.empty((N, N, N), np.uint32), np.zeros(int(counts[0]), sr.NODE), np.zeros(int(counts[1]), sr.BRANCH)
    library().sk_copy(labels, nodes.ctypes.data_as(C.c_void_p), branches.ctypes.data_as(C.c_void_p))
    return labels, nodes, branches, tuple(int(v) for v in counts[2:])


def prune(grid, max_len345):
    """(grid after the prune, branches removed, voxels removed) by the product's own routines"""
    g = np.array(grid, np.uint8, order="C")
    removed = np.zeros(2, np.uint64)
    rc = library().sk_prune(g, g.shape[0], int(max_len345), removed)
    assert rc == 0, rc
    return g, int(removed[0]), int(removed[1])
