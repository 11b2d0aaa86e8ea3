"""The product's line-of-sight routines on the CPU: tests/hostcheck/sight_check.cpp (which includes csrc/dxv_sight.h) compiled into a small
library of its own, the way tests/access_host.py compiles the access's."""
import ctypes as C
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADERS = ("dxv_sight.h", "dxv_fill.h", "dxv_thickness.h", "dxv_solid.h", "dxv_scratch.h", "dxv_types.h")
_LIB = None


def library():
    global _LIB
    if _LIB is None:
        src = os.path.join(ROOT, "tests", "hostcheck", "sight_check.cpp")
        so = os.path.join(ROOT, "tests", "hostcheck", "libsightcheck.so")
        deps = [src] + [os.path.join(ROOT, "dxrvoxelizer_amd", "csrc", h) for h in HEADERS]
        if not os.path.exists(so) or os.path.getmtime(so) < max(os.path.getmtime(d) for d in deps):
            subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-Wall", "-Werror", "-Wno-unknown-pragmas", "-o", so, src])
        L = C.CDLL(so)
        u8 = np.ctypeslib.ndpointer(np.uint8, flags="C")
        u32 = np.ctypeslib.ndpointer(np.uint32, flags="C")
        u64 = np.ctypeslib.ndpointer(np.uint64, flags="C")
        L.sc_sight.argtypes = [u8, C.c_uint32, C.c_int, C.c_uint32, C.c_uint32, u32, u64]
        L.sc_sight.restype = C.c_int
        L.sc_sight_fill.argtypes = [u8, C.c_uint32, C.c_int, C.c_uint32, u32]
        L.sc_sight_fill.restype = C.c_int
        L.sc_valid.argtypes = [C.c_uint32, C.c_int, C.c_uint32]
        L.sc_bit.argtypes = [C.c_int, C.c_int, C.c_int]
        L.sc_bit.restype = L.sc_max_n.restype = L.sc_all.restype = L.sc_group.restype = C.c_uint32
        L.sc_group.argtypes = [C.c_uint32, C.c_uint32]
        L.sc_carve.argtypes = [C.c_uint32, C.c_uint32, C.c_uint64, C.c_uint64, C.POINTER(C.c_int), u64]
        L.sc_carve.restype = C.c_uint64
        _LIB = L
    return _LIB


def tally_dict(words):
    return {"members": int(words[0]), "seen": words[1:28].copy(), "neither": words[28:41].copy(), "count": words[41:68].copy()}


def sight(grid, of, directions, group=0):
    """(map uint32 [N, N, N], tally {members, seen [27], neither [13], count [27]}) by the product's own routines, run word by word; group:
    option sightgroup, the lanes of a row group at the least"""
    g = np.ascontiguousarray(grid, np.uint8)
    N = g.shape[0]
    assert g.shape == (N, N, N)
    out, words = np.empty((N, N, N), np.uint32), np.zeros(68, np.uint64)
    rc = library().sc_sight(g, N, int(of), int(directions), int(group), out, words)
    assert rc == 0, rc
    return out, tally_dict(words)


def sight_fill(grid, of, directions, field):
    """the grid after the edit from `field`, by the product's own routine"""
    g = np.ascontiguousarray(grid, np.uint8).copy()
    rc = library().sc_sight_fill(g, g.shape[0], int(of), int(directions), np.ascontiguousarray(field, np.uint32))
    assert rc == 0, rc
    return g


def carve(N, directions, base=0, capacity=0):
    """(bytes taken, fits, the three blocks' addresses) of sight_carve over `capacity` bytes at `base`"""
    fits, offsets = C.c_int(), np.zeros(3, np.uint64)
    used = library().sc_carve(N, int(directions), base, capacity, C.byref(fits), offsets)
    return int(used), bool(fits.value), [int(o) for o in offsets]
