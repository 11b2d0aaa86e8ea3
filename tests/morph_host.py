"""The product's morphology routines on the CPU: tests/hostcheck/morph_check.cpp (which includes csrc/dxv_morph.h) compiled into a small
library of its own, the way tests/fill_host.py compiles the fill's."""
import ctypes as C
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_LIB = None


def library():
    global _LIB
    if _LIB is None:
        src = os.path.join(ROOT, "tests", "hostcheck", "morph_check.cpp")
        so = os.path.join(ROOT, "tests", "hostcheck", "libmorphcheck.so")
        deps = [src] + [os.path.join(ROOT, "dxrvoxelizer_amd", "csrc", h) for h in ("dxv_morph.h", "dxv_fill.h", "dxv_solid.h", "dxv_types.h")]
        if not os.path.exists(so) or os.path.getmtime(so) < max(os.path.getmtime(d) for d in deps):
            subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-fopenmp", "-ffp-contract=off", "-Wall", "-Werror",
                                   "-Wno-unknown-pragmas", "-o", so, src])
        L = C.CDLL(so)
        L.mc_morph.argtypes = [np.ctypeslib.ndpointer(np.uint8, flags="C"), C.c_uint32, C.c_int, C.c_uint32, C.c_int, C.POINTER(C.c_uint64)]
        L.mc_morph.restype = C.c_int
        L.mc_isqrt.argtypes = [C.c_uint32]
        L.mc_isqrt.restype = C.c_uint32
        L.mc_shifted.argtypes = [C.c_uint64, C.c_uint64, C.c_uint64, C.c_uint32]
        L.mc_shifted.restype = C.c_uint64
        L.mc_threshold.argtypes = [C.c_int32, C.c_uint32, C.c_int]
        L.mc_threshold.restype = C.c_uint32
        L.mc_form.argtypes = [C.c_uint32, C.c_int]
        L.mc_planes_max_radius_sq.restype = C.c_uint32
        L.mc_half_erodes.argtypes = [C.c_int, C.c_uint32]
        _LIB = L
    return _LIB


def morph(grid, op, r2, eight_at_once=True):
    """(the morphed uint8 [N, N, N] grid by the product's own routines, voxels set, voxels cleared)"""
    out = np.ascontiguousarray(grid, np.uint8).copy()
    N = out.shape[0]
    assert out.shape == (N, N, N)
    counts = (C.c_uint64 * 2)()
    assert library().mc_morph(out, N, int(op), int(r2), int(bool(eight_at_once)), counts) == 0
    return out, int(counts[0]), int(counts[1])
