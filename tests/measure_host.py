"""The product's measure routines on the CPU: tests/hostcheck/measure_check.cpp (which includes csrc/dxv_measure.h) compiled into a small library
of its own, the way tests/thin_host.py compiles the thin's."""
import ctypes as C
import os
import subprocess

import numpy as np

import measure_restated as ms

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_LIB = None


def library():
    global _LIB
    if _LIB is None:
        src = os.path.join(ROOT, "tests", "hostcheck", "measure_check.cpp")
        so = os.path.join(ROOT, "tests", "hostcheck", "libmeasurecheck.so")
        deps = [src] + [os.path.join(ROOT, "dxrvoxelizer_amd", "csrc", h) for h in ("dxv_measure.h", "dxv_components.h", "dxv_fill.h", "dxv_solid.h", "dxv_types.h")]
        if not os.path.exists(so) or os.path.getmtime(so) < max(os.path.getmtime(d) for d in deps):
            subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-Wall", "-Werror", "-Wno-unknown-pragmas", "-o", so, src])
        L = C.CDLL(so)
        L.mc_measure.argtypes = [np.ctypeslib.ndpointer(np.uint8, flags="C"), C.c_uint32, C.c_int, C.c_uint32, np.ctypeslib.ndpointer(np.uint32, flags="C"), C.c_uint32,
                                 C.c_void_p]
        L.mc_measure.restype = C.c_int
        L.mc_run.argtypes = [C.c_uint64, C.c_uint64, C.c_uint64, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p]
        L.mc_run.restype = None
        for name in ("mc_record_bytes", "mc_max_n"):
            getattr(L, name).restype = C.c_uint32
        _LIB = L
    return _LIB


def measure(grid, of, connectivity, labels, K):
    """[K + 1] of measure_restated.RECORD by the product's own routines, from a grid and the labels of its labelling"""
    g = np.ascontiguousarray(grid, np.uint8)
    N = g.shape[0]
    assert g.shape == (N, N, N) and library().mc_record_bytes() == ms.RECORD.itemsize
    table = np.empty(K + 1, ms.RECORD)
    rc = library().mc_measure(g, N, int(of), int(connectivity), np.ascontiguousarray(labels, np.uint32), int(K), table.ctypes.data_as(C.c_void_p))
    assert rc == 0, rc
    return table


def run(prev, cur, nxt, connectivity, s, length, x0, y, z):
    """the twelve values of one run of a row that stands alone, as a RECORD"""
    rec = np.zeros(1, ms.RECORD)
    library().mc_run(prev, cur, nxt, connectivity, s, length, x0, y, z, rec.ctypes.data_as(C.c_void_p))
    return rec[0]
