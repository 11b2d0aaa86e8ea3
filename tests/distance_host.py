"""The product's distance-field scans on the CPU: tests/hostcheck/distance_check.cpp (which includes csrc/dxv_distance.h) compiled into a
small library of its own, the way conftest's hostcheck fixture compiles tests/hostcheck/hostcheck.cpp."""
import ctypes as C
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_LIB = None


def library():
    global _LIB
    if _LIB is None:
        src = os.path.join(ROOT, "tests", "hostcheck", "distance_check.cpp")
        so = os.path.join(ROOT, "tests", "hostcheck", "libdistancecheck.so")
        deps = [src] + [os.path.join(ROOT, "dxrvoxelizer_amd", "csrc", h) for h in ("dxv_distance.h", "dxv_types.h")]
        if not os.path.exists(so) or os.path.getmtime(so) < max(os.path.getmtime(d) for d in deps):
            subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-fopenmp", "-ffp-contract=off", "-Wall", "-Werror",
                                   "-Wno-unknown-pragmas", "-o", so, src])
        L = C.CDLL(so)
        L.dc_distance.argtypes = [np.ctypeslib.ndpointer(np.uint8, flags="C"), C.c_uint32, C.c_int, C.c_void_p]
        L.dc_distance.restype = C.c_int
        _LIB = L
    return _LIB


def distance(grid, fmt=0):
    """the field of a uint8 [N, N, N] grid by the product's own scans: int32 (fmt 0) or float32 (fmt 1) [z, y, x]"""
    grid = np.ascontiguousarray(grid, np.uint8)
    N = grid.shape[0]
    assert grid.shape == (N, N, N)
    out = np.empty((N, N, N), np.float32 if fmt else np.int32)
    assert library().dc_distance(grid, N, fmt, out.ctypes.data_as(C.c_void_p)) == 0
    return out
