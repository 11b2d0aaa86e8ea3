"""Library-event times of the line-of-sight map (dxv_sight_info; option events) on the bunny and the torus-1M at 256^3 and the bunny at 512^3:
the empty space of the filled conservative surface (Voxelize(N, MODE_SURFACE); Fill()) for all 26 directions, for one axis pair (+z, -z) and
for a single direction (-z: rays from above).  A run is best of 3 by the whole call's time.  From the same process, as yardsticks and no
gates: dxv_fill on the same grid (the operator whose masks and column passes the sweep resembles), and the compulsory traffic of the call --
N^3 bytes of grid read, 4 N^3 bytes of map written, the mask and the planes written and read once (1 + planes bits per voxel, twice) -- over
5 TB/s; `of_floor` is that time over the measured one.  One JSON line per (mesh, grid, directions).

Every grid is a process of its own under a time limit of its own (mesh, launch and fill included).  A process that meets its time limit or
fails ends the whole measurement.  Nothing is tried again.

usage: sight_times.py [--quick] [--out profiles/sight_times.jsonl]      (--quick: the bunny at 64^3 alone, a rehearsal)"""
import json
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, ".."))

GRIDS = (("bunny", 256), ("torus1m", 256), ("bunny", 512))
REPS = 3
RUN_PROCESS_LIMIT_S = 150
PEAK_BYTES_PER_S = 5.0e12


def child(mesh, N):
    import dxrvoxelizer_amd as dxv
    from bench import make_mesh
    vb, ib = make_mesh(mesh)[:2]
    v = dxv.Voxelizer(0)
    up, down = 1 << dxv.sight_bit(0, 0, 1), 1 << dxv.sight_bit(0, 0, -1)
    requests = (("all 26", dxv.SIGHT_ALL), ("axis z", up | down), ("from above", down))
    try:
        v.InitFromArrays(vb, ib, gridDim=N)
        fill_ms = None
        for _ in range(REPS):                                           # (a fill edits the grid: each repetition fills a fresh launch)
            v.Voxelize(N, dxv.MODE_SURFACE)
            v.Fill()
            ms = v.fill_info()[0]
            fill_ms = ms if fill_ms is None or ms < fill_ms else fill_ms
        for name, directions in requests:
            best = None
            for _ in range(REPS):
                v.Sight(dxv.COMP_EMPTY, directions, sync=False)
                v.Sync()
                ms = v.SightInfo()["ms"]
                best = ms if best is None or ms < best else best
            tally = v.SightTally()
            planes = bin(directions).count("1")
            row_words = (N + 63) // 64
            mask_bytes = N * N * row_words * 8
            traffic = N ** 3 + 4 * N ** 3 + 2 * mask_bytes * (1 + planes)
            floor_ms = traffic / PEAK_BYTES_PER_S * 1e3
            print(json.dumps({"mesh": mesh, "grid": N, "kind": "empty", "directions": name, "planes": planes, "members": tally["members"],
                              "hidden": int(tally["count"][0]), "best_axis": dxv.sight_axes(tally)[0]["axis"] if directions == dxv.SIGHT_ALL else None,
                              "sight_ms": round(best, 4), "fill_ms": round(fill_ms, 4), "over_fill": round(best / fill_ms, 2) if fill_ms > 0 else None,
                              "compulsory_bytes": traffic, "floor_ms_at_5TBps": round(floor_ms, 4), "of_floor": round(floor_ms / best, 3) if best > 0 else None}), flush=True)
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
