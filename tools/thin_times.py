"""Library-event times of topology-preserving thinning (dxv_thin_info, option events): both kinds on the filled conservative surface
(Voxelize(N, MODE_SURFACE); Fill()) of bunny at 256^3 and torus-1M at 512^3, at thinrounds 1, 4, 8, 16 and 64 -- the iterations of one batch; a
thin that needs more is continued where its frame is synchronised, so a small batch pays a host round trip per batch and a large one pays for the
launches of iterations behind the fixed point, which return at once.  The best of 3 of each (each a Voxelize + Fill + Thin, synchronised before
the next).  One JSON line per (mesh, grid, kind, thinrounds): ms, iterations, voxels removed, ms per iteration, ns per voxel removed, and what the
last quarter of the iterations removed -- the tail, in which every sub-iteration still walks every word.

usage: thin_times.py [--quick] [--out profiles/thin_times.jsonl]      (--quick: bunny at 64^3 only, a rehearsal)"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, ".."))
import dxrvoxelizer_amd as dxv  # noqa: E402
from bench import make_mesh  # noqa: E402

CASES = [("bunny", 256), ("torus1m", 512)]
ROUNDS = (1, 4, 8, 16, 64)
KINDS = (("curve", dxv.THIN_CURVE), ("kernel", dxv.THIN_KERNEL))
REPS = 3


def main():
    out = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else None
    lines = []
    for name, N in [("bunny", 64)] if "--quick" in sys.argv else CASES:
        vb, ib = make_mesh(name)[:2]
        v = dxv.Voxelizer(0)
        try:
            v.InitFromArrays(vb, ib, gridDim=N)
            v.Voxelize(N, dxv.MODE_SURFACE)
            v.Fill()
            solid = v.CountSolid()
            for tag, kind in KINDS:
                v.set_option("thinrounds", 0)
                v.Voxelize(N, dxv.MODE_SURFACE)
                v.Fill()
                v.Thin(kind)
                iterations = v.thin_info()[1]
                v.Voxelize(N, dxv.MODE_SURFACE)
                v.Fill()
                v.Thin(kind, max(1, iterations * 3 // 4))
                early = v.thin_info()[2]
                for rounds in ROUNDS:
                    v.set_option("thinrounds", rounds)
                    ms = []
                    for _ in range(REPS):
                        v.Voxelize(N, dxv.MODE_SURFACE)
                        v.Fill()
                        v.Thin(kind)
                        ms.append(v.thin_info()[0])
                    _, its, removed, converged = v.thin_info()
                    rec = {"mesh": name, "grid": N, "solid": solid, "kind": tag, "thinrounds": rounds, "ms": round(min(ms), 4), "ms_all": [round(m, 4) for m in ms],
                           "iterations": its, "removed": removed, "converged": converged, "left": solid - removed,
                           "ms_per_iteration": round(min(ms) / its, 4), "ns_per_voxel_removed": round(min(ms) * 1e6 / max(removed, 1), 3),
                           "removed_by_last_quarter_of_iterations": removed - early}
                    lines.append(json.dumps(rec))
                    print(lines[-1], flush=True)
        finally:
            v.close()
    if out:
        with open(out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
