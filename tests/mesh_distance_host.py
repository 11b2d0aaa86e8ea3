"""The product's mesh distance routine on the CPU: tests/hostcheck/mesh_distance_check.cpp (which includes csrc/dxv_mesh_distance.h)
compiled into a small library of its own, the way tests/distance_host.py compiles the grid field's scans."""
import ctypes as C
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_LIB = None
_F = np.ctypeslib.ndpointer(np.float32, flags="C")
_U = np.ctypeslib.ndpointer(np.uint32, flags="C")


def library():
    global _LIB
    if _LIB is None:
        src = os.path.join(ROOT, "tests", "hostcheck", "mesh_distance_check.cpp")
        so = os.path.join(ROOT, "tests", "hostcheck", "libmeshdistancecheck.so")
        deps = [src] + [os.path.join(ROOT, "dxrvoxelizer_amd", "csrc", h) for h in ("dxv_mesh_distance.h", "dxv_types.h")]
        if not os.path.exists(so) or os.path.getmtime(so) < max(os.path.getmtime(d) for d in deps):
            subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-fopenmp", "-ffp-contract=off", "-Wall", "-Werror",
                                   "-Wno-unknown-pragmas", "-o", so, src])
        L = C.CDLL(so)
        L.mc_brute.argtypes = [_F, C.c_uint32, _F, _U, C.c_uint32, C.c_float, _F, _U]
        L.mc_brute.restype = C.c_int
        L.mc_walk.argtypes = [_F, C.c_uint32, _F, _U, C.c_uint32, C.c_float, C.c_float, C.c_float, _F, _U]
        L.mc_walk.restype = C.c_int
        L.mc_margin.argtypes = [_F, _F, C.POINTER(C.c_float), C.POINTER(C.c_float)]
        L.mc_margin.restype = None
        L.mc_cap.argtypes = [C.c_uint32, C.c_uint32]
        L.mc_cap.restype = C.c_float
        L.mc_value.argtypes = [_F, np.ctypeslib.ndpointer(np.uint8, flags="C"), C.c_size_t, C.c_int, C.c_uint32, _F]
        L.mc_value.restype = None
        _LIB = L
    return _LIB


def _args(points, tris, index):
    points = np.ascontiguousarray(points, np.float32).reshape(-1, 3)
    tris = np.ascontiguousarray(tris, np.float32).reshape(-1, 3, 3)
    index = np.arange(len(tris), dtype=np.uint32) if index is None else np.ascontiguousarray(index, np.uint32)
    return points, tris, index, np.empty(len(points), np.float32), np.empty(len(points), np.uint32)


def margin(tris):
    """(rel, abs) of the product's cull rule for these triangles' root box"""
    t = np.ascontiguousarray(tris, np.float32).reshape(-1, 3)
    rel, ab = C.c_float(), C.c_float()
    library().mc_margin(np.ascontiguousarray(t.min(0)), np.ascontiguousarray(t.max(0)), C.byref(rel), C.byref(ab))
    return rel.value, ab.value


def brute(points, tris, index=None, cap=np.inf):
    points, tris, index, d2, tri = _args(points, tris, index)
    assert library().mc_brute(points, len(points), tris, index, len(tris), cap, d2, tri) == 0
    return d2, tri


def walk(points, tris, index=None, cap=np.inf, rel=None, ab=None):
    """through the hierarchy, with the product's cull constants unless rel / ab are given"""
    points, tris, index, d2, tri = _args(points, tris, index)
    r0, a0 = margin(tris)
    height = library().mc_walk(points, len(points), tris, index, len(tris), cap, r0 if rel is None else rel, a0 if ab is None else ab, d2, tri)
    assert height >= 1, height
    return d2, tri


def cap(N, band):
    return np.float32(library().mc_cap(N, band))


def value(d2, solid, fmt, N):
    d2 = np.ascontiguousarray(d2, np.float32).reshape(-1)
    out = np.empty_like(d2)
    library().mc_value(d2, np.ascontiguousarray(solid, np.uint8).reshape(-1), d2.size, fmt, N, out)
    return out
