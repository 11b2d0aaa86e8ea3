#!/usr/bin/env python3
"""What the lists' integer filter lets through to the triangle step, per 4x4x4 brick, from the host replay of the lists kernel's loop
(tests/hostcheck/filter_check.cpp: the product's own __host__ __device__ code in lockstep for the 64 rays of a brick, start table on).
CPU only.   usage: filter_stats.py MESH N R [every n-th brick layer = 32]
Per brick: triangle tests, tests that hit, the misses split into radial (the line through the centre passes through the triangle) and
lateral (it does not; exact double-precision test), the lateral ones by how far outside the triangle the line passes (-min barycentric,
bands 0.02 / 0.05 / 0.1 / 0.25), scan and triangle rounds; the lists' entries and those without an edge; and the same replay with a
PERFECT filter (an entry passes only if its triangle is hit) -- the floor no encoding of the entries gets under.  One JSON line."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

NAMES = ["bricks", "scan_rounds", "triangle_rounds", "triangle_tests", "tests_that_hit", "radial_misses", "lateral_misses_lt_0.02",
         "lateral_misses_lt_0.05", "lateral_misses_lt_0.1", "lateral_misses_lt_0.25", "lateral_misses_beyond", "entries_looked_at",
         "entries_passed", "flushes", "live_rays"]
LATERAL = [n for n in NAMES if n.startswith("lateral_")]


def library():
    """the check library, built like tests/conftest.py builds libhostcheck.so"""
    d = os.path.join(ROOT, "tests", "hostcheck")
    src, so = os.path.join(d, "filter_check.cpp"), os.path.join(d, "libfiltercheck.so")
    deps = [src, os.path.join(d, "hostcheck.cpp"), os.path.join(d, "start_table_check.cpp")] + [
        os.path.join(ROOT, "dxrvoxelizer_amd", "csrc", h) for h in ("dxv_math.h", "dxv_trace.h", "dxv_types.h", "dxv_dirmap.h", "dxv_raycast.h", "dxv_policy.h")]
    if not os.path.exists(so) or os.path.getmtime(so) < max(os.path.getmtime(p) for p in deps):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-fopenmp", "-ffp-contract=off", "-mavx2", "-mfma",
                               "-Wno-unknown-pragmas", "-o", so, src])
    L = C.CDLL(so)
    f32p, u32p, u8p = (np.ctypeslib.ndpointer(t, flags="C") for t in (np.float32, np.uint32, np.uint8))
    u64p, f64p = np.ctypeslib.ndpointer(np.uint64, flags="C"), np.ctypeslib.ndpointer(np.float64, flags="C")
    L.hc_scene_create.restype = C.c_void_p
    L.hc_scene_create.argtypes = [f32p, C.c_uint32, u32p, C.c_uint32, f32p]
    L.hc_scene_destroy.argtypes = [C.c_void_p]
    L.hc_dirmap_build.argtypes = [C.c_void_p, C.c_uint32]
    L.hc_dirmap_build.restype = C.c_uint64
    L.hc_dirmap_get.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
    L.hc_voxelize.argtypes = [C.c_void_p, C.c_uint32, C.c_int, C.c_uint32, C.c_uint32, C.c_int, u8p, C.c_void_p]
    L.st_table.argtypes = [C.c_void_p, u32p]
    L.st_voxelize.argtypes = [C.c_void_p, C.c_uint32, C.c_int, C.c_void_p, u8p, C.c_void_p]
    L.fc_filter_stats.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, u32p, C.c_int, C.c_int, u64p]
    L.fc_edge_census.argtypes = [C.c_void_p, u64p]
    L.fc_edge_cells.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, u8p, u8p, f64p, C.POINTER(C.c_int32)]
    L.fc_edge_cells.restype = C.c_uint32
    return L


def replay(L, h, N, R, bstep):
    """{"entries", "entries_without_edge", "shipped": {...}, "perfect_filter": {...}} for the lists of R texels built on scene h"""
    n = L.hc_dirmap_build(h, R)
    starts = np.zeros(6 * R * R, np.uint32)
    L.st_table(h, starts)
    census = np.zeros(2, np.uint64)
    L.fc_edge_census(h, census)
    res = {"entries": int(n), "entries_without_edge": int(census[1])}
    for which, perfect in (("shipped", 0), ("perfect_filter", 1)):
        out = np.zeros(20, np.uint64)
        L.fc_filter_stats(h, N, bstep, starts, 1, perfect, out)
        w = float(out[0]) or 1.0
        per = {k: round(float(out[i]) / w, 3) for i, k in enumerate(NAMES) if i}
        per["lateral_misses"] = round(sum(float(out[NAMES.index(k)]) for k in LATERAL) / w, 3)
        res[which] = {"per_brick": per, "bricks": int(out[0]), "tests_that_hit_total": int(out[4]),
                      "lateral_misses_total": int(sum(int(out[NAMES.index(k)]) for k in LATERAL)), "longest_triangle_step_rounds": int(out[15])}
    return res


def main():
    name, N, R = sys.argv[1], int(sys.argv[2]), int(sys.argv[3])
    bstep = int(sys.argv[4]) if len(sys.argv) > 4 else 32
    from oracle import orc       # (only for the bound of the mesh: test infrastructure, like this tool)
    from bench import make_mesh
    L = library()
    vb, ib, _ = make_mesh(name)
    _, b = orc.bound(vb)
    h = L.hc_scene_create(np.ascontiguousarray(vb, np.float32), len(vb), np.ascontiguousarray(ib, np.uint32), len(ib) // 3, b)
    res = {"mesh": name, "N": N, "R": R, "every_nth_brick_layer": bstep}
    res.update(replay(L, h, N, R, bstep))
    L.hc_scene_destroy(h)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
