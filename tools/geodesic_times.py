"""Library-event times of the geodesic distance (dxv_geodesic_info, dxv_geodesic_work_info; option events) on the bunny at 256^3 and 512^3: on the
solid of the filled conservative surface (Voxelize(N, MODE_SURFACE); Fill()) and on that grid's empty space, seeded from the border and from the
single voxel [smallest member index], under both metrics.  A run is best of 3 by the whole call's time; rounds, tiles run, the most live tiles
of a round and the rounds with fewer than 1024 live tiles are that run's.  One JSON line per (grid, kind, seeds, metric).  Beside them the one
comparison with a yardstick: Geodesic(EMPTY, FACES, BORDER) on the conservative surface itself -- it reaches exactly the set dxv_fill floods --
over dxv_fill's time on the same grid, as a ratio.

Every grid is a process of its own under a time limit of its own (mesh, launch and fill included).  A process that meets its time limit or
fails ends the whole measurement.  Nothing is tried again.

usage: geodesic_times.py [--quick] [--out profiles/geodesic_times.jsonl]      (--quick: 64^3 alone, a rehearsal)"""
import json
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, ".."))

GRIDS = (256, 512)
REPS = 3
RUN_PROCESS_LIMIT_S = 150


def child(N):
    import numpy as np
    import dxrvoxelizer_amd as dxv
    from bench import make_mesh
    vb, ib = make_mesh("bunny")[:2]
    v = dxv.Voxelizer(0)

    def best_of(of, metric, seeds):
        best = None
        for _ in range(REPS):
            v.Geodesic(of, metric, seeds, sync=False)
            v.Sync()
            info, work = v.GeodesicInfo(), v.geodesic_work_info()
            if best is None or info["ms"] < best[0]["ms"]:
                best = (info, work)
        return best

    try:
        v.InitFromArrays(vb, ib, gridDim=N)
        v.Voxelize(N, dxv.MODE_SURFACE)
        info, work = best_of(dxv.COMP_EMPTY, dxv.GEO_FACES, "border")
        fill = []
        for _ in range(REPS):
            v.Voxelize(N, dxv.MODE_SURFACE)
            v.Fill(sync=False)
            v.Sync()
            fill.append(v.fill_info())
        fill_ms, fill_rounds = min(fill)
        print(json.dumps({"mesh": "bunny", "grid": N, "what": "Geodesic(EMPTY, FACES, BORDER) on the conservative surface over dxv_fill on the same grid", "geodesic_ms": round(info["ms"], 4),
                          "geodesic_rounds": info["rounds"], "unreached": info["unreached"], "fill_ms": round(fill_ms, 4), "fill_rounds": fill_rounds,
                          "ratio": round(info["ms"] / fill_ms, 2) if fill_ms > 0 else None}), flush=True)
        grid = v.Grid()                                                  # the filled solid
        for kind, of in (("solid", dxv.COMP_SOLID), ("empty", dxv.COMP_EMPTY)):
            members = np.flatnonzero((grid.reshape(-1) != 0) == (of == dxv.COMP_SOLID))
            for seeds_name, seeds in (("border", "border"), ("single", members[:1].astype(np.uint32))):
                for metric_name, metric in (("faces", dxv.GEO_FACES), ("chamfer", dxv.GEO_CHAMFER)):
                    info, work = best_of(of, metric, seeds)
                    rounds = max(info["rounds"], 1)
                    print(json.dumps({"mesh": "bunny", "grid": N, "kind": kind, "members": int(len(members)), "seeds": seeds_name, "metric": metric_name, "ms": round(info["ms"], 4),
                                      "rounds": info["rounds"], "tiles_run": work["tiles_run"], "live_tiles_per_round": round(work["tiles_run"] / rounds, 1),
                                      "most_live_tiles": work["most_live_tiles"], "rounds_below_1024_live_tiles": work["sparse_rounds"], "seeds_used": info["seeds_used"],
                                      "reached": info["reached"], "unreached": info["unreached"], "farthest": info["farthest"]}), flush=True)
    finally:
        v.close()


def main():
    if "--child" in sys.argv:
        child(int(sys.argv[sys.argv.index("--child") + 1]))
        return
    out = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else None
    lines = []

    def save():
        if out:
            with open(out, "w") as fh:
                fh.write("\n".join(lines) + "\n")

    for N in (64,) if "--quick" in sys.argv else GRIDS:
        try:
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", str(N)], capture_output=True, text=True, timeout=RUN_PROCESS_LIMIT_S)
        except subprocess.TimeoutExpired as e:
            lines += [line for line in (e.stdout or b"").decode().splitlines() if line.startswith("{")]
            lines.append(json.dumps({"grid": N, "ended": f"the grid's process met its time limit of {RUN_PROCESS_LIMIT_S} s; nothing further was run"}))
            print(lines[-1], flush=True)
            save()
            sys.exit(124)
        got = [line for line in r.stdout.splitlines() if line.startswith("{")]
        lines += got
        print("\n".join(got), flush=True)
        if r.returncode:
            lines.append(json.dumps({"grid": N, "ended": f"exit status {r.returncode}; nothing further was run", "stderr": r.stderr[-500:]}))
            print(lines[-1], flush=True)
            save()
            sys.exit(1)
        save()


if __name__ == "__main__":
    main()
