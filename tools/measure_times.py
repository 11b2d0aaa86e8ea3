"""Library-event times of the integral measures (dxv_measure_ms, option events) beside the labelling they follow (dxv_components_ms of the same
labelling): SOLID 26 and EMPTY 6 of the reference-rule grid of bunny at 256^3 and torus-1M at 512^3 -- a few components, most waves hold one
label and send once per step -- and SOLID 6 of a random grid of density 0.3 at 256^3 written through the frame's grid pointer -- about a
million components, every lane its own label, no wave-wide reduction.  The best of 5 measures of one labelling (the first of them has the
labelling's mask warm in L2, as a caller's has).  One JSON line per case: K, voxels, faces, euler, both times, their ratio, ns per member voxel.

usage: measure_times.py [--quick] [--out profiles/measure_times.jsonl]      (--quick: bunny and the random grid at 64^3 only, a rehearsal)"""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, ".."))
import dxrvoxelizer_amd as dxv  # noqa: E402
from bench import make_mesh  # noqa: E402

CASES = [("bunny", 256), ("torus1m", 512), ("random 0.3", 256)]
REPS = 5


def write_grid(v, grid):
    import torch
    from dxrvoxelizer_amd.slabs import device_grid_tensor
    v.Sync()
    device_grid_tensor(v, "cuda").copy_(torch.from_numpy(np.ascontiguousarray(grid, np.uint8).reshape(-1)))
    torch.cuda.synchronize()


def main():
    import torch
    torch.cuda.init()                                                   # (before the library's own first HIP call: the random grid is written through torch)
    out = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else None
    lines = []
    for name, N in [("bunny", 64), ("random 0.3", 64)] if "--quick" in sys.argv else CASES:
        random = name.startswith("random")
        vb, ib = make_mesh("bunny" if random else name)[:2]
        v = dxv.Voxelizer(0)
        try:
            v.InitFromArrays(vb, ib, gridDim=N)
            v.Voxelize(N)
            if random:
                write_grid(v, (np.random.default_rng(N).random((N, N, N)) < float(name.split()[1])).astype(np.uint8))
            for of, conn, tag in ((dxv.COMP_SOLID, 6, "solid/6"),) if random else ((dxv.COMP_SOLID, 26, "solid/26"), (dxv.COMP_EMPTY, 6, "empty/6")):
                v.Components(of, conn, sync=False)
                v.Sync()
                comp = v.components_ms()
                ms = []
                for _ in range(REPS):
                    v.Measure(sync=False)
                    v.Sync()
                    ms.append(v.measure_ms())
                t = v.MeasureTable()
                rec = {"grid_of": name, "grid": N, "labelling": tag, "components": len(t) - 1, "voxels": int(t[0]["voxels"]), "faces": int(t[0]["faces"]),
                       "euler": int(t[0]["euler"]), "measure_ms": round(min(ms), 4), "measure_ms_all": [round(m, 4) for m in ms], "components_ms": round(comp, 4),
                       "measure_over_components": round(min(ms) / comp, 3) if comp else None, "ns_per_member_voxel": round(min(ms) * 1e6 / max(int(t[0]["voxels"]), 1), 4)}
                lines.append(json.dumps(rec))
                print(lines[-1], flush=True)
        finally:
            v.close()
    if out:
        with open(out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
