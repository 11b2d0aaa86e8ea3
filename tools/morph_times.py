"""Library-event times of morphology by the Euclidean ball (dxv_morph_info, option events) beside the distance field of the same grid
(dxv_distance_ms): what a caller who thresholds dxv_distance pays today.  One process; mode-0 grids of bunny at 256^3 and torus-1M at 512^3;
every operation at radius_sq 1, 9, 64, 256, 400, 576, 784, 1024 and 4096, in BOTH forms (option morphform: 1 = bit planes, 2 = distance field
+ threshold), so that the radius at which the library switches from one to the other rests on numbers from both sides; the best of 5 of
each (each a Voxelize + Morph, synchronised before the next).  One JSON line per (mesh, grid, radius_sq, form): the four times,
distance_ms (best of 5), the ratios, the form the library picks by itself at that radius, and the morph's scratch bytes per voxel.

usage: morph_times.py [--quick] [--out profiles/morph_times.jsonl]      (--quick: bunny at 64^3 only, a rehearsal)"""
import json
import math
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, ".."))
import dxrvoxelizer_amd as dxv  # noqa: E402
from bench import make_mesh  # noqa: E402

CASES = [("bunny", 256), ("torus1m", 512)]
RADII = (1, 9, 64, 256, 400, 576, 784, 1024, 4096)
FORMS = ((1, "planes"), (2, "field"))
SWITCH = 1024               # kMorphPlanesMaxRadiusSq of csrc/dxv_morph.h: the planes up to it, the field above
OPS = (("dilate", dxv.MORPH_DILATE), ("erode", dxv.MORPH_ERODE), ("open", dxv.MORPH_OPEN), ("close", dxv.MORPH_CLOSE))
REPS = 5


def main():
    out = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else None
    lines = []
    for name, N in [("bunny", 64)] if "--quick" in sys.argv else CASES:
        vb, ib = make_mesh(name)[:2]
        v = dxv.Voxelizer(0)
        try:
            v.InitFromArrays(vb, ib, gridDim=N)
            dist = []
            for _ in range(REPS):
                v.Voxelize(N)
                v.DistanceField(dxv.DIST_SQ_I32, sync=False)
                v.Sync()
                dist.append(v.distance_ms())
            solid = v.CountSolid()
            for r2 in RADII:
                for form, name_of_form in FORMS:
                    v.set_option("morphform", form)
                    rec = {"mesh": name, "grid": N, "solid": solid, "radius_sq": r2, "form": name_of_form,
                           "picked_by_default": (form == 1) == (r2 <= SWITCH), "distance_ms": round(min(dist), 4)}
                    for tag, op in OPS:
                        ms = []
                        for _ in range(REPS):
                            v.Voxelize(N)
                            v.Morph(op, r2)
                            ms.append(v.morph_info()[0])
                        rec[tag + "_ms"] = round(min(ms), 4)
                        rec[tag + "_over_distance"] = round(min(ms) / min(dist), 3)
                        rec[tag + "_set_cleared"] = list(v.morph_info()[1:])
                    bits = 3 + math.isqrt(r2)
                    rec["scratch_bytes_per_voxel"] = [bits / 8, (bits + 1) / 8] if form == 1 else [10.0, 10.0]      # DILATE / ERODE, OPEN / CLOSE
                    lines.append(json.dumps(rec))
                    print(lines[-1], flush=True)
        finally:
            v.close()
    if out:
        with open(out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
