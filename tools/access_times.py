"""Library-event times of the access radius and the intrusion map (dxv_access_info, dxv_access_work_info; option events) on the bunny and the
torus-1M at 256^3 and the bunny at 512^3: the empty space of the filled conservative surface (Voxelize(N, MODE_SURFACE); Fill()) from the border,
connectivity 6, at caps 65 and 257, with and without the intrusion map.  A run is best of 3 by the whole call's time; rounds, tiles run, the
most live tiles of a round and the rounds with fewer than 1024 live tiles are that run's.  From the same process, as yardsticks and no gates:
dxv_distance (the field both share), dxv_geodesic FACES on the same seeds (the same round structure) and dxv_thickness at the same cap (the
same paint).  The shares of a call: field = dxv_distance's time; rounds = the call without the intrusion map less the field (init, rounds,
tally and A's histogram); paint = the call with the intrusion map less the call without.  One JSON line per (mesh, grid, cap).

Every grid is a process of its own under a time limit of its own (mesh, launch and fill included).  A process that meets its time limit or
fails ends the whole measurement.  Nothing is tried again.

usage: access_times.py [--quick] [--out profiles/access_times.jsonl]      (--quick: the bunny at 64^3 alone, a rehearsal)"""
import json
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, ".."))

GRIDS = (("bunny", 256), ("torus1m", 256), ("bunny", 512))
CAPS = (65, 257)
REPS = 3
RUN_PROCESS_LIMIT_S = 150


def child(mesh, N):
    import dxrvoxelizer_amd as dxv
    from bench import make_mesh
    vb, ib = make_mesh(mesh)[:2]
    v = dxv.Voxelizer(0)

    def best_of(run, read):
        best = None
        for _ in range(REPS):
            run()
            v.Sync()
            got = read()
            if best is None or got[0] < best[0]:
                best = got
        return best

    try:
        v.InitFromArrays(vb, ib, gridDim=N)
        v.Voxelize(N, dxv.MODE_SURFACE)
        v.Fill()
        field_ms, = best_of(lambda: v.DistanceField(dxv.DIST_SQ_I32, sync=False), lambda: (v.distance_ms(),))
        geo_ms, geo = best_of(lambda: v.Geodesic(dxv.COMP_EMPTY, dxv.GEO_FACES, "border", sync=False), lambda: (v.GeodesicInfo()["ms"], v.GeodesicInfo()))
        for cap in CAPS:
            thick_ms, = best_of(lambda: v.Thickness(dxv.COMP_EMPTY, cap, sync=False), lambda: (v.ThicknessInfo()[0],))
            plain_ms, plain, plain_work = best_of(lambda: v.Access(dxv.COMP_EMPTY, 6, cap, "border", False, sync=False),
                                                  lambda: (v.AccessInfo()["ms"], v.AccessInfo(), v.access_work_info()))
            full_ms, full, work = best_of(lambda: v.Access(dxv.COMP_EMPTY, 6, cap, "border", True, sync=False), lambda: (v.AccessInfo()["ms"], v.AccessInfo(), v.access_work_info()))
            rounds = max(full["rounds"], 1)
            share = {"field": field_ms / full_ms, "rounds": (plain_ms - field_ms) / full_ms, "paint": (full_ms - plain_ms) / full_ms} if full_ms > 0 else {}
            print(json.dumps({"mesh": mesh, "grid": N, "kind": "empty", "seeds": "border", "connectivity": 6, "cap_sq": cap, "members": full["reached"] + full["unreached"],
                              "access_ms": round(plain_ms, 4), "access_intrusion_ms": round(full_ms, 4), "rounds": full["rounds"], "rounds_without_intrusion": plain["rounds"],
                              "tiles_run": work["tiles_run"], "live_tiles_per_round": round(work["tiles_run"] / rounds, 1), "most_live_tiles": work["most_live_tiles"],
                              "rounds_below_1024_live_tiles": work["sparse_rounds"], "seeds_used": full["seeds_used"], "reached": full["reached"], "unreached": full["unreached"],
                              "widest": full["widest"], "share": {k: round(s, 3) for k, s in share.items()}, "distance_ms": round(field_ms, 4), "geodesic_faces_ms": round(geo_ms, 4),
                              "geodesic_rounds": geo["rounds"], "thickness_ms": round(thick_ms, 4),
                              "over_geodesic_plus_thickness": round(full_ms / (geo_ms + thick_ms), 2) if geo_ms + thick_ms > 0 else None}), flush=True)
    finally:
        v.close()


def main():
    if "--child" in sys.argv:
        at = sys.argv.index("--child")
        child(sys.argv[at + 1], int(sys.argv[at + 2]))
        return
    out = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else None
    lines = []

    def save():
        if out:
            with open(out, "w") as fh:
                fh.write("\n".join(lines) + "\n")

    for mesh, N in (("bunny", 64),) if "--quick" in sys.argv else GRIDS:
        try:
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", mesh, str(N)], capture_output=True, text=True, timeout=RUN_PROCESS_LIMIT_S)
        except subprocess.TimeoutExpired as e:
            lines += [line for line in (e.stdout or b"").decode().splitlines() if line.startswith("{")]
            lines.append(json.dumps({"mesh": mesh, "grid": N, "ended": f"the grid's process met its time limit of {RUN_PROCESS_LIMIT_S} s; nothing further was run"}))
            print(lines[-1], flush=True)
            save()
            sys.exit(124)
        got = [line for line in r.stdout.splitlines() if line.startswith("{")]
        lines += got
        print("\n".join(got), flush=True)
        if r.returncode:
            lines.append(json.dumps({"mesh": mesh, "grid": N, "ended": f"exit status {r.returncode}; nothing further was run", "stderr": r.stderr[-500:]}))
            print(lines[-1], flush=True)
            save()
            sys.exit(1)
        save()


if __name__ == "__main__":
    main()
