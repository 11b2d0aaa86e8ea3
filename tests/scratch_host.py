"""The operators' scratch descriptions on the CPU: tests/hostcheck/scratch_check.cpp (which includes the carve functions of csrc/dxv_*.h)
compiled into a small library of its own, the way tests/components_host.py compiles the components."""
import ctypes as C
import glob
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_LIB = None


def library():
    global _LIB
    if _LIB is None:
        src = os.path.join(ROOT, "tests", "hostcheck", "scratch_check.cpp")
        so = os.path.join(ROOT, "tests", "hostcheck", "libscratchcheck.so")
        deps = [src] + glob.glob(os.path.join(ROOT, "dxrvoxelizer_amd", "csrc", "dxv_*.h"))
        if not os.path.exists(so) or os.path.getmtime(so) < max(os.path.getmtime(d) for d in deps):
            subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-Wall", "-Werror", "-Wno-unknown-pragmas", "-o", so, src])
        L = C.CDLL(so)
        L.sc_row.argtypes = [C.c_char_p, C.POINTER(C.c_ulonglong), C.c_ulonglong, C.c_ulonglong, C.c_char_p, C.c_int]
        L.sc_row.restype = C.c_int
        L.sc_oct_levels.argtypes = [C.c_uint32]
        L.sc_oct_levels.restype = C.c_ulonglong
        _LIB = L
    return _LIB


def carve(op, args, base=0, capacity=0):
    """(bytes used, fits, {buffer: offset from base, -1 for null}) of operator `op` carved over `base` (an address that is never
    touched; 0: the sizing run) with `capacity` bytes behind it"""
    a = (C.c_ulonglong * 4)(*(list(args) + [0] * (4 - len(args))))
    out = C.create_string_buffer(4096)
    n = library().sc_row(op.encode(), a, base, capacity, out, len(out))
    assert n > 0, f"scratch_check knows no operator {op!r}"
    used, fits, *rest = out.value.decode().split()
    return int(used), fits == "1", {k: int(v) for k, v in (kv.split("=") for kv in rest)}


def oct_levels(N):
    return int(library().sc_oct_levels(N))
