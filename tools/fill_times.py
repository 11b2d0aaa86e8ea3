"""Library-event times of the exterior flood fill (dxv_fill_info, option events) of the conservative surface (mode 2), beside the
voxelization it sits behind.  One JSON line per case: mesh, grid, voxelize_ms of the same frame, surface and filled voxels, the rounds
the fill took, the median and minimum over standalone fills (each a Voxelize + Fill, synchronised before the next), the byte floor --
2 bytes per voxel, the pack's read and the write-back's write -- at 6.3 TB/s and that floor as a fraction of the measured time.
--cpu: the wall time of the download + scipy.ndimage.label of the same grid on this box, where scipy is present.

usage: fill_times.py [--quick] [--quick512] [--cpu] [--out profiles/fill_times.jsonl]
(--quick: bunny 64^3 only, 3 fills: a rehearsal; --quick512: dragon x9 at 512^3 only, 3 fills: what a kernel trace is taken of)"""
import json
import os
import statistics
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, ".."))
import dxrvoxelizer_amd as dxv  # noqa: E402
from bench import make_mesh  # noqa: E402

CASES = [("bunny", 256), ("torus1m", 512), ("dragon9", 512), ("dragon9", 1024)]
BYTES_PER_VOXEL = 2
HBM_BYTES_PER_MS = 6.3e9


def cpu_seconds(v):
    try:
        from scipy import ndimage
    except ImportError:
        return None
    t0 = time.time()
    grid = v.Grid()
    ndimage.label(grid == 0)
    return round(time.time() - t0, 2)


def main():
    quick = "--quick" in sys.argv
    out = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else None
    cases = [("bunny", 64)] if quick else [("dragon9", 512)] if "--quick512" in sys.argv else CASES
    reps = 3 if quick or "--quick512" in sys.argv else 20
    lines = []
    for name, N in cases:
        vb, ib, _ = make_mesh(name)
        v = dxv.Voxelizer(0)
        v.InitFromArrays(vb, ib, gridDim=N)
        for _ in range(3):
            v.Voxelize(N, dxv.MODE_SURFACE)
        row = {"mesh": name, "tris": int(len(ib) // 3), "grid": N, "voxelize_ms": round(v.stats()["voxelize_ms"], 4), "surface": v.CountSolid()}
        if "--cpu" in sys.argv and N <= 512:
            row["download_and_scipy_label_s"] = cpu_seconds(v)
        floor_ms = BYTES_PER_VOXEL * N ** 3 / HBM_BYTES_PER_MS
        ms, rounds = [], 0
        for i in range(reps + 2):
            v.Voxelize(N, dxv.MODE_SURFACE, sync=False)
            v.Fill(dxv.FILL_SOLID, sync=False)
            v.Sync()
            if i >= 2:
                t, rounds = v.fill_info()
                ms.append(t)
        med = statistics.median(ms)
        row.update({"solid": v.CountSolid(), "rounds": rounds, "fill_ms": round(med, 4), "fill_min_ms": round(min(ms), 4),
                    "byte_floor_ms": round(floor_ms, 4), "floor_over_time": round(floor_ms / med, 3), "fills_per_voxelize": round(med / row["voxelize_ms"], 2)})
        v.close()
        print(json.dumps(row), flush=True)
        lines.append(row)
    if out:
        with open(out, "w") as fh:
            for row in lines:
                fh.write(json.dumps(row) + "\n")


if __name__ == "__main__":
    main()
