"""The product's thickness routines on the CPU: tests/hostcheck/thickness_check.cpp (which includes csrc/dxv_thickness.h and csrc/dxv_distance.h)
compiled into a small library of its own, the way tests/measure_host.py compiles the measure's."""
import ctypes as C
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_LIB = None


def library():
    global _LIB
    if _LIB is None:
        src = os.path.join(ROOT, "tests", "hostcheck", "thickness_check.cpp")
        so = os.path.join(ROOT, "tests", "hostcheck", "libthicknesscheck.so")
        deps = [src] + [os.path.join(ROOT, "dxrvoxelizer_amd", "csrc", h) for h in ("dxv_thickness.h", "dxv_distance.h", "dxv_types.h")]
        if not os.path.exists(so) or os.path.getmtime(so) < max(os.path.getmtime(d) for d in deps):
            subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-Wall", "-Werror", "-Wno-unknown-pragmas", "-o", so, src])
        L = C.CDLL(so)
        L.tc_thickness.argtypes = [np.ctypeslib.ndpointer(np.uint8, flags="C"), C.c_uint32, C.c_int, C.c_uint32, C.c_uint32, np.ctypeslib.ndpointer(np.uint32, flags="C"),
                                   np.ctypeslib.ndpointer(np.uint64, flags="C"), np.ctypeslib.ndpointer(np.uint64, flags="C")]
        L.tc_thickness.restype = C.c_int
        L.tc_max_n.restype = C.c_uint32
        L.tc_isqrt.argtypes = [C.c_uint32]
        L.tc_isqrt.restype = C.c_uint32
        _LIB = L
    return _LIB


def thickness(grid, of, cap_sq, cull=3):
    """(W uint32 [N, N, N], histogram uint64 [cap_sq + 1], (centres painted, work items)) by the product's own routines, run serially"""
    g = np.ascontiguousarray(grid, np.uint8)
    N = g.shape[0]
    assert g.shape == (N, N, N)
    W = np.empty((N, N, N), np.uint32)
    hist = np.empty(cap_sq + 1, np.uint64)
    counters = np.zeros(2, np.uint64)
    rc = library().tc_thickness(g, N, int(of), int(cap_sq), int(cull), W, hist, counters)
    assert rc == 0, rc
    return W, hist, (int(counters[0]), int(counters[1]))
