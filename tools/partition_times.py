"""Library-event times of the maximal-ball partition (dxv_partition_info, dxv_partition_stage_info; options events, partprune, partstages) on the
filled conservative surface (Voxelize(N, MODE_SURFACE); Fill()) of bunny and torus-1M at 256^3 and 512^3, both kinds, cap_sq 17, 65, 257, 1025,
4096 in that order.  Under the default partprune 3 a run is the best of 2 by the whole call's time under partstages = 1; the stages' times and the
counters are that run's; ms_plain is the best of 2 further calls under partstages = 0, what a caller pays; thickness_ms is dxv_thickness on the
same grid, kind and cap, the project's other ball-sized operator.  The single levels (partprune 1, 2) run once each up to cap_sq 257, the plain
ball walk (partprune 0) up to cap_sq 65 at 256^3 and 17 at 512^3: beyond that they are r^3 per voxel by construction.  One JSON line per (grid,
kind, cap_sq, partprune).

Every (grid, kind) is a process of its own under a time limit of its own (mesh, launch and fill included), its caps a LADDER in rising order: a
call that takes over 2 s ends the ladder there, and its line says so.  A process that meets its time limit or fails ends the whole measurement.
Nothing is tried again.

usage: partition_times.py [--quick] [--budget SECONDS] [--out profiles/partition_times.jsonl]
(--quick: bunny at 64^3, caps 17 and 65, a rehearsal; --budget: no further process is started once one could not end within that many seconds)"""
import json
import os
import subprocess
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, ".."))

CASES = [("bunny", 256), ("torus1m", 256), ("bunny", 512), ("torus1m", 512)]
CAPS = (17, 65, 257, 1025, 4096)
REPS = 2
RUN_LIMIT_MS = 2000.0
PROCESS_LIMIT_S = 150


def one(v, of, cap, prune, staged):
    v.set_option("partprune", prune)
    v.set_option("partstages", 1 if staged else 0)
    v.Partition(of, cap, sync=False)
    v.Sync()
    return v.PartitionInfo(), v.partition_stage_info()


def child(name, N, kind, quick):
    import dxrvoxelizer_amd as dxv
    from bench import make_mesh
    vb, ib = make_mesh(name)[:2]
    v = dxv.Voxelizer(0)
    try:
        v.InitFromArrays(vb, ib, gridDim=N)
        v.Voxelize(N, dxv.MODE_SURFACE)
        v.Fill()
        solid = v.CountSolid()
        of = dxv.COMP_SOLID if kind == "solid" else dxv.COMP_EMPTY
        for cap in (17, 65) if quick else CAPS:
            prunes = [3] + ([1, 2] if cap <= 257 else []) + ([0] if cap <= (65 if N <= 256 else 17) else [])
            stop = False
            for prune in prunes:
                best = None
                for _ in range(REPS if prune == 3 else 1):
                    (ms, regions, throats, faces), (stages, cells, voxels) = one(v, of, cap, prune, True)
                    if best is None or ms < best[0]:
                        best = (ms, regions, throats, faces, stages, cells, voxels)
                    if ms > RUN_LIMIT_MS:
                        break
                ms, regions, throats, faces, stages, cells, voxels = best
                rec = {"mesh": name, "grid": N, "solid": solid, "kind": kind, "cap_sq": cap, "partprune": prune, "ms": round(ms, 4), "stages_ms": {k: round(t, 4) for k, t in stages.items()},
                       "regions": regions, "throats": throats, "interface_faces": faces, "cells_tested": cells, "voxels_tested": voxels,
                       "tests_per_s": round((cells + voxels) / (stages["search"] * 1e-3)) if stages["search"] > 0 else None}
                if prune == 3:
                    plain = [one(v, of, cap, 3, False)[0][0] for _ in range(REPS if ms <= RUN_LIMIT_MS else 0)]
                    rec["ms_plain"] = round(min(plain), 4) if plain else None
                    v.Thickness(of, max(cap, 2), sync=False)
                    v.Sync()
                    rec["thickness_ms"] = round(v.ThicknessInfo()[0], 4)
                if ms > RUN_LIMIT_MS:
                    rec["ladder_stopped_here"] = f"over {RUN_LIMIT_MS / 1000:.0f} s"
                    stop = True
                print(json.dumps(rec), flush=True)
                if stop:
                    break
            if stop:
                break
    finally:
        v.close()


def main():
    quick = "--quick" in sys.argv
    if "--child" in sys.argv:
        name, N, kind = sys.argv[sys.argv.index("--child") + 1:][:3]
        child(name, int(N), kind, quick)
        return
    out = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else None
    budget = float(sys.argv[sys.argv.index("--budget") + 1]) if "--budget" in sys.argv else None
    began = time.time()
    lines = []

    def save():
        if out:
            with open(out, "w") as fh:
                fh.write("\n".join(lines) + "\n")

    for name, N in [("bunny", 64)] if quick else CASES:
        for kind in ("solid", "empty"):
            what = {"mesh": name, "grid": N, "kind": kind}
            if budget is not None and time.time() - began + PROCESS_LIMIT_S > budget:
                lines.append(json.dumps(dict(what, ended="not started: the measurement's time budget")))
                print(lines[-1], flush=True)
                save()
                continue
            try:
                r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", name, str(N), kind] + (["--quick"] if quick else []), capture_output=True, text=True,
                                   timeout=PROCESS_LIMIT_S)
            except subprocess.TimeoutExpired as e:
                lines += [line for line in (e.stdout or b"").decode().splitlines() if line.startswith("{")]
                lines.append(json.dumps(dict(what, ended=f"the process met its time limit of {PROCESS_LIMIT_S} s; nothing further was run")))
                print(lines[-1], flush=True)
                save()
                return 1
            got = [line for line in r.stdout.splitlines() if line.startswith("{")]
            lines += got
            print("\n".join(got), flush=True)
            if r.returncode:
                lines.append(json.dumps(dict(what, ended=f"exit status {r.returncode}; nothing further was run", stderr=r.stderr[-500:])))
                print(lines[-1], flush=True)
                save()
                return 1
            save()
    return 0


if __name__ == "__main__":
    sys.exit(main())
