"""Library-event times (stats voxelize_ms, option events) of the surface modes beside the reference rule.  One JSON line per case:
mesh, grid, and for modes 0 (reference), 2 (surface) and 3 (reference + surface) the median and minimum over the timed launches,
the voxel count and, for mode 2, how many triangles take the large-triangle path (box over 64 candidate voxels, from the
restatement's host-side box rule).

usage: surface_times.py [--quick] [--out profiles/surface_times.jsonl]   (--quick: bunny 64^3 only, 3 launches: a rehearsal)"""
import json
import os
import statistics
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, ".."))
import dxrvoxelizer_amd as dxv  # noqa: E402
from bench import make_mesh  # noqa: E402
from dxrvoxelizer_amd import meshes  # noqa: E402

CASES = [("torus1m", 512), ("dragon9", 512), ("bunny", 256), ("cube", 1024), ("tetrahedron", 1024)]


def mesh(name):
    if name in ("cube", "tetrahedron"):
        vb, ib = getattr(meshes, name)()
        return vb, ib
    vb, ib, _ = make_mesh(name)
    return vb, ib


def large_triangles(vb, ib, N):
    """triangles whose candidate box (the kernel's: 1/16 voxel of margin) holds more than 64 voxels"""
    p = np.ascontiguousarray(vb, np.float32).reshape(-1, 6)[:, :3]
    mn, mx = p.min(0), p.max(0)
    c, w = (mx + mn) / np.float32(2), (mx - mn).max() / np.float32(2)
    t = ((p - c) / w)[np.asarray(ib, np.int64).reshape(-1, 3)].astype(np.float64)
    u = (t + 1.0) * N / 2
    u[..., 1] = (1.0 - t[..., 1]) * N / 2
    lo = np.clip(np.floor(u.min(1) - 0.0625), 0, N - 1)
    hi = np.clip(np.floor(u.max(1) + 0.0625), 0, N - 1)
    return int(((hi - lo + 1).prod(1) > 64).sum())


def times(v, N, mode, reps):
    for _ in range(3):
        v.Voxelize(N, mode=mode)
    ms = []
    for _ in range(reps):
        v.Voxelize(N, mode=mode)
        ms.append(v.stats()["voxelize_ms"])
    return {"median_ms": round(statistics.median(ms), 4), "min_ms": round(min(ms), 4), "voxels": v.CountSolid()}


def main():
    quick = "--quick" in sys.argv
    out = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else None
    cases = [("bunny", 64)] if quick else CASES
    reps = 3 if quick else 20
    lines = []
    for name, N in cases:
        vb, ib = mesh(name)
        v = dxv.Voxelizer(0)
        v.InitFromArrays(vb, ib, gridDim=N)                    # (the reference rule's launch as Init prepares it)
        row = {"mesh": name, "tris": int(len(ib) // 3), "grid": N, "large_tris": large_triangles(vb, ib, N)}
        for mode, tag in ((0, "reference"), (2, "surface"), (3, "reference_surface")):
            row[tag] = times(v, N, mode, reps)
        v.close()
        print(json.dumps(row), flush=True)
        lines.append(row)
    if out:
        with open(out, "w") as fh:
            for row in lines:
                fh.write(json.dumps(row) + "\n")


if __name__ == "__main__":
    main()
