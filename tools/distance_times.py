"""Library-event times of the distance field (dxv_distance_ms, option events) beside the voxelization it sits next to.  One JSON line
per case: mesh, grid, voxelize_ms of the same frame, and for both formats the median and minimum over standalone fields (each
synchronised before the next), the bytes the three passes move per voxel at the least (17) and the time those bytes
take at 6.3 TB/s as a fraction of the measured time.  --cpu: the wall time of scipy.ndimage's exact transform of the same grid
(both kinds) on this box, where scipy is present.

usage: distance_times.py [--quick] [--quick512] [--cpu] [--out profiles/distance_times.jsonl]
(--quick: bunny 64^3 only, 3 fields: a rehearsal; --quick512: dragon x9 at 512^3 only, 3 fields: what a kernel trace is taken of)"""
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
BYTES_PER_VOXEL = 1 + 2 + 2 + 4 + 4 + 4        # x: grid read, 16-bit written; y: 16-bit read, squares written; z: squares read, field written
HBM_BYTES_PER_MS = 6.3e9


def cpu_seconds(grid):
    try:
        from scipy import ndimage
    except ImportError:
        return None
    solid = grid != 0
    t0 = time.time()
    ndimage.distance_transform_edt(solid)
    ndimage.distance_transform_edt(~solid)
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
            v.Voxelize(N)
        row = {"mesh": name, "tris": int(len(ib) // 3), "grid": N, "voxelize_ms": round(v.stats()["voxelize_ms"], 4), "solid": v.CountSolid(),
               "bytes_per_voxel": BYTES_PER_VOXEL}
        floor_ms = BYTES_PER_VOXEL * N ** 3 / HBM_BYTES_PER_MS
        for fmt, tag in ((dxv.DIST_SQ_I32, "sq_i32"), (dxv.DIST_F32, "f32")):
            ms = []
            for i in range(reps + 2):
                v.DistanceField(fmt, sync=False)
                v.Sync()
                if i >= 2:
                    ms.append(v.distance_ms())
            med = statistics.median(ms)
            row[tag] = {"median_ms": round(med, 4), "min_ms": round(min(ms), 4), "hbm_floor_ms": round(floor_ms, 4),
                        "floor_over_time": round(floor_ms / med, 3), "fields_per_voxelize": round(med / row["voxelize_ms"], 2)}
        if "--cpu" in sys.argv and N <= 512:
            row["scipy_edt_both_kinds_s"] = cpu_seconds(v.Grid())
        v.close()
        print(json.dumps(row), flush=True)
        lines.append(row)
    if out:
        with open(out, "w") as fh:
            for row in lines:
                fh.write(json.dumps(row) + "\n")


if __name__ == "__main__":
    main()
