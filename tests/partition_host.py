"""The product's partition routines on the CPU: tests/hostcheck/partition_check.cpp (which includes csrc/dxv_partition.h, csrc/dxv_thickness.h and
csrc/dxv_distance.h) compiled into a small library of its own, the way tests/thickness_host.py compiles the thickness's."""
import ctypes as C
import os
import subprocess

import numpy as np

from partition_restated import REGION, THROAT

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FORWARD, REVERSED, SHUFFLED = 0, 1, 2
_LIB = None


def library():
    global _LIB
    if _LIB is None:
        src = os.path.join(ROOT, "tests", "hostcheck", "partition_check.cpp")
        so = os.path.join(ROOT, "tests", "hostcheck", "libpartitioncheck.so")
        deps = [src] + [os.path.join(ROOT, "dxrvoxelizer_amd", "csrc", h) for h in ("dxv_partition.h", "dxv_thickness.h", "dxv_distance.h", "dxv_types.h")]
        if not os.path.exists(so) or os.path.getmtime(so) < max(os.path.getmtime(d) for d in deps):
            subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-Wall", "-Werror", "-Wno-unknown-pragmas", "-o", so, src])
        L = C.CDLL(so)
        L.pc_partition.argtypes = [np.ctypeslib.ndpointer(np.uint8, flags="C"), C.c_uint32, C.c_int, C.c_uint32, C.c_uint32, C.c_int, C.c_int, np.ctypeslib.ndpointer(np.uint64, flags="C")]
        L.pc_partition.restype = C.c_int
        L.pc_fetch.argtypes = [np.ctypeslib.ndpointer(np.uint32, flags="C"), C.c_void_p, C.c_void_p]
        L.pc_fetch.restype = None
        _LIB = L
    return _LIB


def partition(grid, of, cap_sq, prune=3, order=FORWARD, want_throats=True):
    """(labels uint32 [N, N, N], table REGION [K], throats THROAT [T], (interface faces, mip cells tested, voxels tested)) by the product's own
    routines, run serially"""
    g = np.ascontiguousarray(grid, np.uint8)
    N = g.shape[0]
    assert g.shape == (N, N, N)
    counts = np.zeros(5, np.uint64)
    rc = library().pc_partition(g, N, int(of), int(cap_sq), int(prune), int(order), int(bool(want_throats)), counts)
    assert rc == 0, rc
    labels = np.empty((N, N, N), np.uint32)
    table, throats = np.zeros(int(counts[0]), REGION), np.zeros(int(counts[1]), THROAT)
    library().pc_fetch(labels, table.ctypes.data_as(C.c_void_p), throats.ctypes.data_as(C.c_void_p))
    return labels, table, throats, (int(counts[2]), int(counts[3]), int(counts[4]))
