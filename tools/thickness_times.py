"""Library-event times of the local thickness (dxv_thickness_info, dxv_thickness_stage_info; options events, thickstages) on the filled
conservative surface (Voxelize(N, MODE_SURFACE); Fill()) of bunny at 256^3 and torus-1M at 512^3, both kinds, cap_sq 17, 65, 257, 1025, 4096 in
that order, under every thickcull (3 first).  A run is best of 3 by the whole call's time under thickstages = 1; the stages' times, the counters
and the paint's rate are that run's; ms_plain is the best of 3 further calls under thickstages = 0, what a caller pays.  One JSON line per
(grid, kind, cap_sq, thickcull): ms, the six stages, centres painted, work items, voxels the paint tested, atomics it sent, atomics per second and
their bytes per second (4 each) beside the only yardstick there is, the chip's 1.3 TB/s of float add atomics.

Every run is a process of its own under a time limit of its own (mesh, launch and fill included).  A LADDER is the caps of one (grid, kind) in
rising order: a run whose call takes over 2 s ends that ladder there -- the other kind of the same grid still runs --, and its line says so.  A
process that meets its time limit or fails ends the whole measurement.  Nothing is tried again.

usage: thickness_times.py [--quick] [--out profiles/thickness_times.jsonl]      (--quick: bunny at 64^3, caps 17 and 65, a rehearsal)"""
import json
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, ".."))

CASES = [("bunny", 256), ("torus1m", 512)]
CAPS = (17, 65, 257, 1025, 4096)
CULLS = (3, 2, 1, 0)
REPS = 3
RUN_LIMIT_MS = 2000.0
RUN_PROCESS_LIMIT_S = 90
FLOAT_ADD_BYTES_PER_S = 1.3e12


def child(name, N, kind, cap, cull):
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
        v.set_option("thickcull", cull)
        v.set_option("thickstages", 1)
        best = None
        for _ in range(REPS):
            v.Thickness(of, cap, sync=False)
            v.Sync()
            ms, centres, items = v.ThicknessInfo()
            stages, tested, sent = v.thickness_stage_info()
            if best is None or ms < best[0]:
                best = (ms, centres, items, stages, tested, sent)
            if ms > RUN_LIMIT_MS:
                break
        ms, centres, items, stages, tested, sent = best
        plain = []
        v.set_option("thickstages", 0)
        for _ in range(REPS if ms <= RUN_LIMIT_MS else 0):
            v.Thickness(of, cap, sync=False)
            v.Sync()
            plain.append(v.ThicknessInfo()[0])
        paint = stages["paint"]
        rec = {"mesh": name, "grid": N, "solid": solid, "kind": kind, "cap_sq": cap, "thickcull": cull, "ms": round(ms, 4), "ms_plain": round(min(plain), 4) if plain else None,
               "stages_ms": {k: round(t, 4) for k, t in stages.items()}, "centres_painted": centres, "work_items": items, "voxels_tested": tested,
               "atomics_sent": sent, "atomics_per_s": round(sent / (paint * 1e-3)) if paint > 0 else None,
               "atomic_bytes_per_s_over_float_add": round(4 * sent / (paint * 1e-3) / FLOAT_ADD_BYTES_PER_S, 4) if paint > 0 else None,
               "tested_per_s": round(tested / (paint * 1e-3)) if paint > 0 else None}
        if ms > RUN_LIMIT_MS:
            rec["ladder_stopped_here"] = f"over {RUN_LIMIT_MS / 1000:.0f} s"
        print(json.dumps(rec), flush=True)
    finally:
        v.close()


def main():
    if "--child" in sys.argv:
        name, N, kind, cap, cull = sys.argv[sys.argv.index("--child") + 1:][:5]
        child(name, int(N), kind, int(cap), int(cull))
        return
    out = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else None
    quick = "--quick" in sys.argv
    lines = []

    def save():
        if out:
            with open(out, "w") as fh:
                fh.write("\n".join(lines) + "\n")

    for name, N in [("bunny", 64)] if quick else CASES:
        for kind in ("solid", "empty"):
            stopped = False
            for cap in (17, 65) if quick else CAPS:
                for cull in CULLS:
                    what = {"mesh": name, "grid": N, "kind": kind, "cap_sq": cap, "thickcull": cull}
                    try:
                        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", name, str(N), kind, str(cap), str(cull)], capture_output=True, text=True,
                                           timeout=RUN_PROCESS_LIMIT_S)
                    except subprocess.TimeoutExpired:
                        lines.append(json.dumps(dict(what, ended=f"the run's process met its time limit of {RUN_PROCESS_LIMIT_S} s; nothing further was run")))
                        print(lines[-1], flush=True)
                        save()
                        return
                    got = [line for line in r.stdout.splitlines() if line.startswith("{")]
                    if r.returncode or len(got) != 1:
                        lines.append(json.dumps(dict(what, ended=f"exit status {r.returncode}; nothing further was run", stderr=r.stderr[-500:])))
                        print(lines[-1], flush=True)
                        save()
                        return
                    lines += got
                    print(got[0], flush=True)
                    save()
                    if "ladder_stopped_here" in got[0]:
                        stopped = True
                        break
                if stopped:
                    break


if __name__ == "__main__":
    main()
