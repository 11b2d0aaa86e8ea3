"""The product's access routines on the CPU: tests/hostcheck/access_check.cpp (which includes csrc/dxv_access.h, and tests/hostcheck/thickness_check.cpp
for the fields and the paint) compiled into a small library of its own, the way tests/geodesic_host.py compiles the geodesic's."""
import ctypes as C
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BORDER, LIST, MASK = 0, 1, 2
HEADERS = ("dxv_access.h", "dxv_geodesic.h", "dxv_thickness.h", "dxv_distance.h", "dxv_types.h")
_LIB = None


def library():
    global _LIB
    if _LIB is None:
        src = os.path.join(ROOT, "tests", "hostcheck", "access_check.cpp")
        so = os.path.join(ROOT, "tests", "hostcheck", "libaccesscheck.so")
        deps = [src, os.path.join(ROOT, "tests", "hostcheck", "thickness_check.cpp")] + [os.path.join(ROOT, "dxrvoxelizer_amd", "csrc", h) for h in HEADERS]
        if not os.path.exists(so) or os.path.getmtime(so) < max(os.path.getmtime(d) for d in deps):
            subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-Wall", "-Werror", "-Wno-unknown-pragmas", "-o", so, src])
        L = C.CDLL(so)
        u64 = np.ctypeslib.ndpointer(np.uint64, flags="C")
        L.ac_access.argtypes = [np.ctypeslib.ndpointer(np.uint8, flags="C"), C.c_uint32, C.c_int, C.c_int, C.c_uint32, C.c_int, C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32,
                                np.ctypeslib.ndpointer(np.uint32, flags="C"), C.c_void_p, u64, u64, u64, u64]
        L.ac_access.restype = C.c_int
        L.ac_max_n.restype = C.c_uint32
        L.ac_touch.argtypes = [C.c_uint32, C.c_uint32, C.c_uint32, C.c_int]
        L.ac_touch.restype = C.c_uint32
        L.ac_valid.argtypes = [C.c_uint32, C.c_int, C.c_int, C.c_uint32]
        _LIB = L
    return _LIB


def access(grid, of, connectivity, cap_sq, seeds="border", intrusion=True, cull=3, shuffle=0):
    """{A, I (None without intrusion), hist_a, hist_i, tally {seeds_used, reached, unreached, widest, widest_voxel}, rounds, tiles_run} by the
    product's own routines, run serially; shuffle != 0: every round's tiles in an order shuffled from that seed.  seeds: "border", an array of
    voxel indices, or N^3 values of which the non-zero ones are seeds."""
    g = np.ascontiguousarray(grid, np.uint8)
    N = g.shape[0]
    assert g.shape == (N, N, N)
    if isinstance(seeds, str):
        kind, ptr, count, keep = BORDER, None, 0, None
    else:
        s = np.asarray(seeds)
        if s.ndim == 3:
            keep = np.ascontiguousarray(s != 0, np.uint8)
            kind, count = MASK, 0
        else:
            keep = np.ascontiguousarray(s, np.uint32)
            kind, count = LIST, len(keep)
        ptr = keep.ctypes.data_as(C.c_void_p)
    A = np.empty((N, N, N), np.uint32)
    I = np.empty((N, N, N), np.uint32) if intrusion else None
    hist_a, hist_i = np.zeros(cap_sq + 1, np.uint64), np.zeros(cap_sq + 1, np.uint64)
    tally, work = np.zeros(5, np.uint64), np.zeros(2, np.uint64)
    rc = library().ac_access(g, N, int(of), int(connectivity), int(cap_sq), kind, ptr, count, int(cull), int(shuffle), A, I.ctypes.data_as(C.c_void_p) if intrusion else None,
                             hist_a, hist_i, tally, work)
    assert rc == 0, rc
    names = ("seeds_used", "reached", "unreached", "widest", "widest_voxel")
    return {"A": A, "I": I, "hist_a": hist_a, "hist_i": hist_i if intrusion else None, "tally": dict(zip(names, (int(v) for v in tally))), "rounds": int(work[0]),
            "tiles_run": int(work[1])}
