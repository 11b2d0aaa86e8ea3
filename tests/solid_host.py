"""The library's solid rule on the CPU: tests/hostcheck/solid_check.cpp (which includes csrc/dxv_solid.h) compiled into a small library
of its own, the way tests/fill_host.py compiles the flood fill."""
import ctypes as C
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_LIB = None
_U8 = np.ctypeslib.ndpointer(np.uint8, flags="C")
_U64 = np.ctypeslib.ndpointer(np.uint64, flags="C")


def library():
    global _LIB
    if _LIB is None:
        src = os.path.join(ROOT, "tests", "hostcheck", "solid_check.cpp")
        so = os.path.join(ROOT, "tests", "hostcheck", "libsolidcheck.so")
        deps = [src] + [os.path.join(ROOT, "dxrvoxelizer_amd", "csrc", h) for h in ("dxv_solid.h", "dxv_types.h")]
        if not os.path.exists(so) or os.path.getmtime(so) < max(os.path.getmtime(d) for d in deps):
            subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-Wall", "-Werror", "-Wno-unknown-pragmas", "-o", so, src])
        L = C.CDLL(so)
        L.sc_words.argtypes = [_U64, C.c_size_t, _U8, _U64]
        L.sc_words.restype = None
        L.sc_tail_bits.argtypes = [_U8, C.c_size_t]
        L.sc_tail_bits.restype = C.c_uint32
        L.sc_pack_and_count.argtypes = [_U8, C.c_size_t, _U8]
        L.sc_pack_and_count.restype = C.c_uint64
        _LIB = L
    return _LIB


def words(w):
    """(solid_bits, solid_marks) of every 64-bit word of w: uint8 [n], uint64 [n]"""
    w = np.ascontiguousarray(w, np.uint64).reshape(-1)
    bits, marks = np.empty(len(w), np.uint8), np.empty(len(w), np.uint64)
    library().sc_words(w, len(w), bits, marks)
    return bits, marks


def tail_bits(voxels):
    """the scalar solid_bits of a run of bytes (it looks at the first eight at the most)"""
    voxels = np.ascontiguousarray(voxels, np.uint8).reshape(-1)
    return int(library().sc_tail_bits(voxels, len(voxels)))


def pack_and_count(grid):
    """(packed uint8 [ceil(n / 8)], count) of n grid bytes in the kernels' order: 16-byte pieces, then the ragged end"""
    grid = np.ascontiguousarray(grid, np.uint8).reshape(-1)
    packed = np.full((len(grid) + 7) // 8, 0xAA, np.uint8)              # (every byte must be written)
    count = library().sc_pack_and_count(grid, len(grid), packed)
    return packed, int(count)
