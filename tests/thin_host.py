"""The product's thinning routines on the CPU: tests/hostcheck/thin_check.cpp (which includes csrc/dxv_thin.h) compiled into a small library of
its own, the way tests/morph_host.py compiles the morph's."""
import ctypes as C
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_LIB = None


def library():
    global _LIB
    if _LIB is None:
        src = os.path.join(ROOT, "tests", "hostcheck", "thin_check.cpp")
        so = os.path.join(ROOT, "tests", "hostcheck", "libthincheck.so")
        deps = [src] + [os.path.join(ROOT, "dxrvoxelizer_amd", "csrc", h) for h in ("dxv_thin.h", "dxv_morph.h", "dxv_fill.h", "dxv_solid.h", "dxv_types.h")]
        if not os.path.exists(so) or os.path.getmtime(so) < max(os.path.getmtime(d) for d in deps):
            subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-Wall", "-Werror", "-Wno-unknown-pragmas", "-o", so, src])
        L = C.CDLL(so)
        L.tc_thin.argtypes = [np.ctypeslib.ndpointer(np.uint8, flags="C"), C.c_uint32, C.c_int, C.c_uint32, C.c_int, C.POINTER(C.c_uint64)]
        L.tc_thin.restype = C.c_int
        for name in ("tc_T26", "tc_T6"):
            getattr(L, name).argtypes = [C.c_uint32]
            getattr(L, name).restype = C.c_uint32
        L.tc_simple.argtypes = [C.c_uint32]
        L.tc_keeps.argtypes = [C.c_int, C.c_uint32]
        L.tc_decide.argtypes = [np.ctypeslib.ndpointer(np.uint32, flags="C"), C.c_size_t, np.ctypeslib.ndpointer(np.uint32, flags="C")]
        L.tc_decide.restype = None
        L.tc_three.argtypes = [C.c_uint64, C.c_uint64, C.c_uint64, C.c_uint32]
        L.tc_three.restype = C.c_uint32
        L.tc_batch.argtypes = [C.c_uint32, C.c_uint32]
        for name in ("tc_batch", "tc_rounds_default", "tc_rounds_max", "tc_max_n"):
            getattr(L, name).restype = C.c_uint32
        _LIB = L
    return _LIB


def thin(grid, kind, max_iterations=0, eight_at_once=True):
    """(the thinned uint8 [N, N, N] grid by the product's own routines, iterations, voxels removed, converged)"""
    out = np.ascontiguousarray(grid, np.uint8).copy()
    N = out.shape[0]
    assert out.shape == (N, N, N)
    info = (C.c_uint64 * 3)()
    assert library().tc_thin(out, N, int(kind), int(max_iterations), int(bool(eight_at_once)), info) == 0
    return out, int(info[0]), int(info[1]), bool(info[2])


def decide(cfg):
    """per configuration: (simple, kept by CURVE, T26, T6) by the header's routines"""
    cfg = np.ascontiguousarray(cfg, np.uint32)
    out = np.zeros(len(cfg), np.uint32)
    library().tc_decide(cfg, len(cfg), out)
    return (out & 1) != 0, (out & 2) != 0, (out >> 8) & 0xff, (out >> 16) & 0xff
