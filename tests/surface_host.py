"""The surface pass's candidate enumeration on the CPU: tests/hostcheck/surface_check.cpp (which includes csrc/dxv_surface.h) compiled into
a small library of its own, the way tests/access_host.py compiles the access routines."""
import ctypes as C
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NO_BOX, SMALL, LARGE = 0, 1, 2
HEADERS = ("dxv_surface.h", "dxv_math.h", "dxv_types.h")
_LIB = None


def library():
    global _LIB
    if _LIB is None:
        src = os.path.join(ROOT, "tests", "hostcheck", "surface_check.cpp")
        so = os.path.join(ROOT, "tests", "hostcheck", "libsurfacecheck.so")
        deps = [src] + [os.path.join(ROOT, "dxrvoxelizer_amd", "csrc", h) for h in HEADERS]
        if not os.path.exists(so) or os.path.getmtime(so) < max(os.path.getmtime(d) for d in deps):
            subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-Wall", "-Werror", "-Wno-unknown-pragmas", "-o", so, src])
        L = C.CDLL(so)
        L.sc_surface.argtypes = [np.ctypeslib.ndpointer(np.float32, flags="C"), C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_int, C.c_int,
                                 np.ctypeslib.ndpointer(np.uint8, flags="C"), np.ctypeslib.ndpointer(np.uint32, flags="C")]
        L.sc_surface.restype = C.c_int
        _LIB = L
    return _LIB


def surface(tris, N, z0=0, nz=None, zblock=None, zperiod=None, force_large=False, old_walk=False):
    """(grid uint8 [nz, N, N], info uint32 [T, 3] = path, candidates tested, candidates accepted per triangle) of normalised triangles
    (T, 3, 3), made as the two kernels make it.  The partition: a slab of nz slices from z0 (default: the whole grid), or nz local slices in
    blocks of zblock every zperiod.  force_large: every triangle through the column walk; old_walk: the walk without the far-vertex limit."""
    t = np.ascontiguousarray(tris, np.float32).reshape(-1, 9)
    nz = N - z0 if nz is None else nz
    zblock = nz if zblock is None else zblock
    zperiod = zblock if zperiod is None else zperiod
    grid, info = np.zeros((nz, N, N), np.uint8), np.zeros((len(t), 3), np.uint32)
    rc = library().sc_surface(t, len(t), N, z0, nz, zblock, zperiod, int(force_large), int(old_walk), grid, info)
    assert rc == 0, rc
    return grid, info
