"""The product's isosurface routines on the CPU: tests/hostcheck/isosurface_check.cpp (which includes csrc/dxv_isosurface.h) compiled into a
small library of its own, the way tests/distance_host.py compiles the distance scans."""
import ctypes as C
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_LIB = None
_F = np.ctypeslib.ndpointer(np.float32, flags="C")


def library():
    global _LIB
    if _LIB is None:
        src = os.path.join(ROOT, "tests", "hostcheck", "isosurface_check.cpp")
        so = os.path.join(ROOT, "tests", "hostcheck", "libisosurfacecheck.so")
        deps = [src] + [os.path.join(ROOT, "dxrvoxelizer_amd", "csrc", h) for h in ("dxv_isosurface.h", "dxv_types.h")]
        if not os.path.exists(so) or os.path.getmtime(so) < max(os.path.getmtime(d) for d in deps):
            subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-Wall", "-Werror",
                                   "-Wno-unknown-pragmas", "-o", so, src])
        L = C.CDLL(so)
        L.ic_extract.argtypes = [_F, C.c_uint32, C.c_float, C.c_float, C.c_int, _F, C.c_void_p, C.c_void_p, C.c_void_p]
        L.ic_extract.restype = C.c_int
        _LIB = L
    return _LIB


def extract(field, iso=0.0, P=1.0, space=0, bound=None):
    """(vb [V, 6] float32, ib [3T] uint32) of a float32 [N, N, N] field by the product's own routines, in the kernels' order"""
    field = np.ascontiguousarray(field, np.float32)
    N = field.shape[0]
    assert field.shape == (N, N, N)
    bound = np.ascontiguousarray([0, 0, 0, 1] if bound is None else bound, np.float32)
    counts = np.zeros(2, np.uint64)
    args = (field, N, float(iso), float(P), int(space), bound, counts.ctypes.data_as(C.c_void_p))
    assert library().ic_extract(*args, None, None) == 0
    vb, ib = np.empty((int(counts[0]), 6), np.float32), np.empty(3 * int(counts[1]), np.uint32)
    assert library().ic_extract(*args, vb.ctypes.data_as(C.c_void_p), ib.ctypes.data_as(C.c_void_p)) == 0
    return vb, ib
