#!/usr/bin/env python3
"""Host replay of the lists kernel's loop per 4x4x4 brick (tests/hostcheck/start_table_check.cpp: the product's own __host__ __device__
code, in lockstep for the 64 rays of a brick): what a wave issues -- scan rounds and scan load instructions, search loads, triangle
rounds, flushes -- with the scan beginning where the start search ends ("shipped") and no earlier than the start table's start
("table").  CPU only.   usage: round_stats.py MESH N R [every n-th brick layer = 16]"""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

NAMES = ["bricks", "scan_rounds", "scan_rounds_with_loads", "scan_load_instructions", "search_load_instructions", "search_loads_all_lanes",
         "triangle_rounds", "flushes", "entries_looked_at", "entries_passed", "cooperative_rounds", "bricks_that_scan", "rays_moved_by_table",
         "live_rays"]


def library():
    """the check library, built like tests/conftest.py builds libhostcheck.so"""
    d = os.path.join(ROOT, "tests", "hostcheck")
    src, so = os.path.join(d, "start_table_check.cpp"), os.path.join(d, "libstartcheck.so")
    deps = [src, os.path.join(d, "hostcheck.cpp")] + [os.path.join(ROOT, "dxrvoxelizer_amd", "csrc", h)
                                                       for h in ("dxv_math.h", "dxv_trace.h", "dxv_types.h", "dxv_dirmap.h", "dxv_raycast.h", "dxv_policy.h")]
    if not os.path.exists(so) or os.path.getmtime(so) < max(os.path.getmtime(p) for p in deps):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-fopenmp", "-ffp-contract=off", "-mavx2", "-mfma",
                               "-Wno-unknown-pragmas", "-o", so, src])
    L = C.CDLL(so)
    f32p, u32p = np.ctypeslib.ndpointer(np.float32, flags="C"), np.ctypeslib.ndpointer(np.uint32, flags="C")
    L.hc_scene_create.restype = C.c_void_p
    L.hc_scene_create.argtypes = [f32p, C.c_uint32, u32p, C.c_uint32, f32p]
    L.hc_scene_destroy.argtypes = [C.c_void_p]
    L.hc_dirmap_build.argtypes = [C.c_void_p, C.c_uint32]
    L.hc_dirmap_build.restype = C.c_uint64
    L.hc_dirmap_get.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
    L.st_table.argtypes = [C.c_void_p, u32p]
    L.st_buckets.restype = C.c_uint32
    L.st_offset.argtypes = [C.c_uint32, C.c_uint32, C.c_uint32, C.c_float]
    L.st_offset.restype = C.c_uint32
    L.st_probe.argtypes = [C.c_void_p, u32p, C.c_void_p]
    L.st_probe_raw.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, u32p, C.c_void_p]
    L.st_voxelize.argtypes = [C.c_void_p, C.c_uint32, C.c_int, C.c_void_p, np.ctypeslib.ndpointer(np.uint8, flags="C"), C.c_void_p]
    L.st_round_stats.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_int, C.c_void_p]
    return L


def main():
    name, N, R = sys.argv[1], int(sys.argv[2]), int(sys.argv[3])
    bstep = int(sys.argv[4]) if len(sys.argv) > 4 else 16
    from oracle import orc       # (only for the bound of the mesh: test infrastructure, like this tool)
    from bench import make_mesh
    L = library()
    vb, ib, _ = make_mesh(name)
    _, b = orc.bound(vb)
    h = L.hc_scene_create(np.ascontiguousarray(vb, np.float32), len(vb), np.ascontiguousarray(ib, np.uint32), len(ib) // 3, b)
    n = L.hc_dirmap_build(h, R)
    starts = np.zeros(6 * R * R, np.uint32)
    L.st_table(h, starts)
    res = {"mesh": name, "N": N, "R": R, "entries": int(n), "every_nth_brick_layer": bstep, "buckets": int(L.st_buckets())}
    for which, ptr in (("shipped", None), ("table", starts.ctypes.data_as(C.c_void_p))):
        out = np.zeros(len(NAMES), np.uint64)
        L.st_round_stats(h, N, bstep, ptr, 1, out.ctypes.data_as(C.c_void_p))
        w = float(out[0]) or 1.0
        res[which] = {"per_brick": {k: round(float(out[i]) / w, 3) for i, k in enumerate(NAMES) if i}, "bricks": int(out[0])}
    L.hc_scene_destroy(h)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
