"""The product's flood-fill routines on the CPU: tests/hostcheck/fill_check.cpp (which includes csrc/dxv_fill.h) compiled into a small
library of its own, the way tests/distance_host.py compiles the distance scans."""
import ctypes as C
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_LIB = None


def library():
    global _LIB
    if _LIB is None:
        src = os.path.join(ROOT, "tests", "hostcheck", "fill_check.cpp")
        so = os.path.join(ROOT, "tests", "hostcheck", "libfillcheck.so")
        deps = [src] + [os.path.join(ROOT, "dxrvoxelizer_amd", "csrc", h) for h in ("dxv_fill.h", "dxv_solid.h", "dxv_types.h", "dxv_policy.h")]
        if not os.path.exists(so) or os.path.getmtime(so) < max(os.path.getmtime(d) for d in deps):
            subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-fopenmp", "-ffp-contract=off", "-Wall", "-Werror",
                                   "-Wno-unknown-pragmas", "-o", so, src])
        L = C.CDLL(so)
        L.fc_fill.argtypes = [np.ctypeslib.ndpointer(np.uint8, flags="C"), C.c_uint32, C.c_int, C.c_int, C.POINTER(C.c_uint32)]
        L.fc_fill.restype = C.c_int
        L.fc_fill_word.argtypes = [C.c_uint64, C.c_uint64]
        L.fc_fill_word.restype = C.c_uint64
        L.fc_option_accepts.argtypes = [C.c_char_p, C.c_int64]
        L.fc_option_default.argtypes = [C.c_char_p]
        _LIB = L
    return _LIB


def fill(grid, what=0, eight_at_once=True):
    """(the filled uint8 [N, N, N] grid by the product's own routines, the rounds they took -- the confirming one included)"""
    out = np.ascontiguousarray(grid, np.uint8).copy()
    N = out.shape[0]
    assert out.shape == (N, N, N)
    rounds = C.c_uint32()
    assert library().fc_fill(out, N, int(what), int(bool(eight_at_once)), C.byref(rounds)) == 0
    return out, rounds.value
