"""Library-event times of the mesh distance field (dxv_mesh_distance_ms, option events) beside the voxelization and the grid's own
distance field of the same frame.  One JSON line per case: mesh, grid, voxelize_ms, the grid field's median (dxv_distance_ms, float
format), and for band 0 and band 4, with and without triangles, the median and minimum over standalone fields (each synchronised
before the next) of the walk over the hierarchy -- and, where --brute names the case, of the brute-force kernel (option mdistwalk 0,
three fields).  A configuration whose first field takes over 250 ms is timed over 3 fields instead of 20.

usage: mesh_distance_times.py [--quick] [--quick512] [--out profiles/mesh_distance_times.jsonl]
(--quick: bunny 64^3 only, 3 fields: a rehearsal; --quick512: dragon x9 at 512^3 only, 3 fields: what a kernel trace is taken of)"""
import json
import os
import statistics
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, ".."))
import dxrvoxelizer_amd as dxv  # noqa: E402
from bench import make_mesh  # noqa: E402

CASES = [("bunny", 128, True), ("bunny", 256, False), ("torus1m", 512, False), ("dragon9", 512, False)]   # (mesh, grid, brute force too)
BANDS = (0, 4)


def timed(v, reps, call, read):
    ms = []
    for i in range(reps + 2):
        call()
        v.Sync()
        if i >= 2:
            ms.append(read())
        if i == 0 and read() > 250.0:
            reps = min(reps, 3)
        if len(ms) >= reps:
            break
    return {"median_ms": round(statistics.median(ms), 4), "min_ms": round(min(ms), 4), "fields": len(ms)}


def main():
    quick = "--quick" in sys.argv
    out = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else None
    cases = [("bunny", 64, True)] if quick else [("dragon9", 512, False)] if "--quick512" in sys.argv else CASES
    reps = 3 if quick or "--quick512" in sys.argv else 20
    lines = []
    for name, N, brute in cases:
        vb, ib, _ = make_mesh(name)
        v = dxv.Voxelizer(0)
        v.InitFromArrays(vb, ib, gridDim=N)
        for _ in range(3):
            v.Voxelize(N)
        row = {"mesh": name, "tris": int(len(ib) // 3), "grid": N, "voxelize_ms": round(v.stats()["voxelize_ms"], 4), "solid": v.CountSolid()}
        row["grid_distance_f32"] = timed(v, reps, lambda: v.DistanceField(dxv.DIST_F32, sync=False), v.distance_ms)
        for walk, tag in ((1, "walk"), (0, "brute")) if brute else ((1, "walk"),):
            v.set_option("mdistwalk", walk)
            for band in BANDS:
                for tri in (False, True):
                    key = f"{tag}_band{band}" + ("_tri" if tri else "")
                    row[key] = timed(v, reps if walk else 3, lambda: v.MeshDistanceField(dxv.MDIST_VOXELS_F32, band, tri, sync=False), v.mesh_distance_ms)
                    row[key]["per_voxelize"] = round(row[key]["median_ms"] / row["voxelize_ms"], 2)
        v.close()
        print(json.dumps(row), flush=True)
        lines.append(row)
    if out:
        with open(out, "w") as fh:
            for row in lines:
                fh.write(json.dumps(row) + "\n")


if __name__ == "__main__":
    main()
