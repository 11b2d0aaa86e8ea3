"""The product's connected-component routines on the CPU: tests/hostcheck/components_check.cpp (which includes csrc/dxv_components.h)
compiled into a small library of its own, the way tests/fill_host.py compiles the fill."""
import ctypes as C
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RECORD = np.dtype([("first", "<u4"), ("voxels", "<u4"), ("lo", "<u2", (3,)), ("hi", "<u2", (3,)), ("flags", "<u4")])
_LIB = None


def library():
    global _LIB
    if _LIB is None:
        src = os.path.join(ROOT, "tests", "hostcheck", "components_check.cpp")
        so = os.path.join(ROOT, "tests", "hostcheck", "libcomponentscheck.so")
        deps = [src] + [os.path.join(ROOT, "dxrvoxelizer_amd", "csrc", h) for h in ("dxv_components.h", "dxv_fill.h", "dxv_solid.h", "dxv_types.h")]
        if not os.path.exists(so) or os.path.getmtime(so) < max(os.path.getmtime(d) for d in deps):
            subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-Wall", "-Werror", "-Wno-unknown-pragmas", "-o", so, src])
        L = C.CDLL(so)
        L.cc_components.argtypes = [np.ctypeslib.ndpointer(np.uint8, flags="C"), C.c_uint32, C.c_int, C.c_uint32, C.c_int, C.c_int,
                                    np.ctypeslib.ndpointer(np.uint32, flags="C"), C.c_void_p]
        L.cc_components.restype = C.c_longlong
        L.cc_select.argtypes = [C.c_void_p, C.c_uint32, C.c_int, C.c_uint32, np.ctypeslib.ndpointer(np.uint8, flags="C")]
        L.cc_select.restype = C.c_uint32
        L.cc_run_start.argtypes = [C.c_uint64, C.c_uint32]
        L.cc_run_start.restype = C.c_uint32
        L.cc_max_n.restype = C.c_uint32
        _LIB = L
    return _LIB


def components(grid, of=0, connectivity=6, eight_at_once=True, backwards=False):
    """(labels uint32 [N, N, N], table [K] of RECORD) by the product's own routines"""
    g = np.ascontiguousarray(grid, np.uint8)
    N = g.shape[0]
    assert g.shape == (N, N, N)
    labels = np.empty((N, N, N), np.uint32)
    table = np.empty(N ** 3, RECORD)
    K = library().cc_components(g, N, int(of), int(connectivity), int(bool(eight_at_once)), int(bool(backwards)), labels, table.ctypes.data_as(C.c_void_p))
    assert K >= 0
    return labels, table[:K].copy()


def select(table, rule, arg=0):
    """bool [K]: which components the product's rule keeps"""
    t = np.ascontiguousarray(table, RECORD)
    keep = np.zeros(max(len(t), 1), np.uint8)
    kept = library().cc_select(t.ctypes.data_as(C.c_void_p), len(t), int(rule), int(arg), keep)
    keep = keep[:len(t)].astype(bool)
    assert kept == int(keep.sum())
    return keep
