"""Library-event times of the skeleton graph (dxv_skeleton_info; option events) beside dxv_components SOLID at connectivity 26 of the same grid --
the nearest existing operator: the same pack, union-find and stats shape; a yardstick, no gate -- on three grids at 256^3: the bunny thinned to
curves (Voxelize(N, MODE_SURFACE); Fill(); Thin(THIN_CURVE): sparse), the bunny filled and not thinned (one huge node: the union-find's worst
case) and a random grid at density 0.05.  A figure is the best of REPS runs of one process.  One JSON line per grid.

With --kernel-stats FILE --grid N the tool reads the kernel statistics a profiler run of `--child` wrote (a CSV with the columns Name, Calls,
TotalDurationNs) and prints, per grid side, the classify pass alone and the components' pack beside it: mean time and GB/s of mask bytes the
classify pass reads (nine words of its column per mask word) and of grid bytes the pack reads.

Every grid is a process of its own under a time limit of its own (mesh, launch, fill and thin included).  A process that meets its time limit or
fails ends the whole measurement.  Nothing is tried again.

usage: skeleton_times.py [--quick] [--out profiles/skeleton_times.jsonl]      (--quick: at 64^3, a rehearsal)
       skeleton_times.py --child GRID N
       skeleton_times.py --kernel-stats FILE --grid N"""
import csv
import json
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, ".."))

GRIDS = ("bunny thinned", "bunny filled", "random 0.05")
REPS = 5
RUN_PROCESS_LIMIT_S = 200


def child(grid, N):
    import numpy as np
    import torch
    import dxrvoxelizer_amd as dxv
    from dxrvoxelizer_amd.slabs import device_grid_tensor
    from bench import make_mesh
    vb, ib = make_mesh("bunny")[:2]
    v = dxv.Voxelizer(0)

    def best_of(run, read):
        best = None
        for _ in range(REPS):
            run()
            v.Sync()
            got = read()
            if best is None or got < best:
                best = got
        return best

    try:
        v.InitFromArrays(vb, ib, gridDim=N)
        v.Voxelize(N, dxv.MODE_SURFACE)
        if grid == "random 0.05":
            rng = np.random.default_rng(256)
            g = (rng.random((N, N, N)) < 0.05).astype(np.uint8)
            v.Sync()
            device_grid_tensor(v, "cuda").copy_(torch.from_numpy(g.reshape(-1)))
            torch.cuda.synchronize()
        else:
            v.Fill()
            if grid == "bunny thinned":
                v.Thin(dxv.THIN_CURVE)
        comp_ms = best_of(lambda: v.Components(dxv.COMP_SOLID, 26, sync=False), v.components_ms)
        skel_ms = best_of(lambda: v.Skeleton(sync=False), lambda: v.SkeletonInfo()["ms"])
        info = v.SkeletonInfo()
        print(json.dumps({"grid": grid, "side": N, "members": info["end_voxels"] + info["curve_voxels"] + info["junction_voxels"], "nodes": info["nodes"], "branches": info["branches"],
                          "end_voxels": info["end_voxels"], "curve_voxels": info["curve_voxels"], "junction_voxels": info["junction_voxels"], "components": v.components_info()[0],
                          "skeleton_ms": round(skel_ms, 4), "components_ms": round(comp_ms, 4), "skeleton_over_components": round(skel_ms / comp_ms, 2) if comp_ms > 0 else None, "runs": REPS}), flush=True)
    finally:
        v.close()


def kernel_stats(path, N):
    rows = list(csv.DictReader(open(path)))
    W = (N + 63) // 64
    mask_words = N * N * W
    out = {}
    for r in rows:
        name = r.get("Name") or r.get("KernelName") or ""
        calls, total = int(r.get("Calls") or r.get("Count") or 0), float(r.get("TotalDurationNs") or r.get("TotalDuration") or 0)
        if not calls:
            continue
        for key, nbytes in (("k_skel_classify", 9 * 8 * mask_words), ("k_comp_pack", N ** 3)):
            if key in name:
                mean = total / calls
                out[key] = {"calls": calls, "mean_us": round(mean / 1e3, 2), "bytes_read": nbytes, "GB_per_s": round(nbytes / mean, 1)}
    print(json.dumps({"side": N, "kernels": out, "source": "kernel trace, a run of its own"}), flush=True)


def main():
    if "--child" in sys.argv:
        at = sys.argv.index("--child")
        child(sys.argv[at + 1], int(sys.argv[at + 2]))
        return
    if "--kernel-stats" in sys.argv:
        kernel_stats(sys.argv[sys.argv.index("--kernel-stats") + 1], int(sys.argv[sys.argv.index("--grid") + 1]))
        return
    out = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else None
    N = 64 if "--quick" in sys.argv else 256
    lines = []

    def save():
        if out:
            with open(out, "w") as fh:
                fh.write("\n".join(lines) + "\n")

    for grid in GRIDS:
        try:
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", grid, str(N)], capture_output=True, text=True, timeout=RUN_PROCESS_LIMIT_S)
        except subprocess.TimeoutExpired as e:
            lines += [line for line in (e.stdout or b"").decode().splitlines() if line.startswith("{")]
            lines.append(json.dumps({"grid": grid, "side": N, "ended": f"the grid's process met its time limit of {RUN_PROCESS_LIMIT_S} s; nothing further was run"}))
            print(lines[-1], flush=True)
            save()
            sys.exit(124)
        got = [line for line in r.stdout.splitlines() if line.startswith("{")]
        lines += got
        print("\n".join(got), flush=True)
        if r.returncode:
            lines.append(json.dumps({"grid": grid, "side": N, "ended": f"exit status {r.returncode}; nothing further was run", "stderr": r.stderr[-500:]}))
            print(lines[-1], flush=True)
            save()
            sys.exit(1)
        save()


if __name__ == "__main__":
    main()
