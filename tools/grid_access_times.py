#!/usr/bin/env python3
"""The grid accessors' kernels at a size a user runs: K calls each of CountSolid (k_count) and GridBits (k_pack_bits) on the bunny's
N^3 grid, for a run under `rocprofv3 --kernel-trace --stats` (the kernels' device times; the host's times printed here include the
copy back and the synchronisation).  Run alternately with DXV_LIBRARY set to two builds on ONE box for a same-box A/B.
    DXV_LIBRARY=... python tools/grid_access_times.py [N] [K] [tag]"""
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import dxrvoxelizer_amd as dxv  # noqa: E402

N = int(sys.argv[1]) if len(sys.argv) > 1 else 512
K = int(sys.argv[2]) if len(sys.argv) > 2 else 40
tag = sys.argv[3] if len(sys.argv) > 3 else os.path.basename(os.environ.get("DXV_LIBRARY", "libdxv.so"))
d = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests", "golden", "meshes", "bunny.npz"))
v = dxv.Voxelizer(0)
v.InitFromArrays(d["vb"], d["ib"], gridDim=N)
v.Voxelize(N)
out = np.empty((N ** 3 + 7) // 8, np.uint8)


def loop(call):
    for _ in range(5):
        call()
    t = []
    for _ in range(K):
        t0 = time.perf_counter()
        call()
        t.append((time.perf_counter() - t0) * 1e3)
    return round(float(np.median(t)), 4)


count_ms = loop(v.CountSolid)
bits_ms = loop(lambda: v.GridBits(out))
solid = v.CountSolid()
assert solid == int(np.unpackbits(out).sum())
print(json.dumps({"lib": tag, "N": N, "calls": K, "count_call_ms": count_ms, "bits_call_ms": bits_ms, "solid": solid}))
v.close()
