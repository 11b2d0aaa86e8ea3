"""Makes tests/golden/mesh_distance.json and mesh_distance_sample.npz: the mesh distance field of the three asset meshes at 32^3, from the numpy restatement
(tests/mesh_distance_restated.py: every triangle for every voxel, 0.7 - 3.3 G pairs per mesh -- minutes of CPU, once).  CPU only:

    python tests/gen_mesh_distance_fixtures.py

Recorded per mesh, for band 0 and band 3 and both formats: the SHA-256 of the field's MAGNITUDE (float32 [z, y, x]; the sign is the grid's
and is checked against the grid the device made), its min, max and sum (float64 of the float32 values, as hex), the SHA-256 of tri(p),
and -- in the .npz beside it, <mesh>_band<B>_bits / _tri -- a seeded sample of 4 096 voxels (flat indices from
default_rng(seed).choice, sorted) with the bits of the magnitude in voxel units and the triangle there, so that a failure says where."""
import hashlib
import json
import multiprocessing as mp
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
GOLD = os.path.join(HERE, "golden")
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)

import mesh_distance_restated as mr  # noqa: E402
from surface_restated import normalised_tris  # noqa: E402

N = 32
BANDS = (0, 3)
MESHES = ("bunny", "dragon", "turingbowl")
SAMPLE, SEED = 4096, 20261017


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def _part(args):
    points, tris = args
    return mr.nearest(points, tris)


def summary(d2, tri, band):
    """what the fixture records of one (mesh, band): d2 float32 (V,), tri uint32 (V,) of the unbanded field"""
    cap = mr.cap_of(N, band)
    if cap is not None:
        tri = np.where(cap < d2, np.uint32(mr.NO_TRIANGLE), tri).astype(np.uint32)
        d2 = np.minimum(d2, cap)
    none = np.zeros(d2.size, np.uint8)
    out = {"tri_sha256": sha(tri)}
    for fmt, name in ((mr.VOXELS_F32, "voxels"), (mr.UNITS_F32, "units")):
        mag = mr.value(d2, none, fmt, N)
        out[name] = {"sha256": sha(mag), "min": float(mag.min()).hex(), "max": float(mag.max()).hex(), "sum": float(mag.sum(dtype=np.float64)).hex()}
    where = np.sort(np.random.default_rng(SEED).choice(d2.size, SAMPLE, replace=False))
    return out, mr.value(d2, none, mr.VOXELS_F32, N).view(np.uint32)[where], tri[where]


def main():
    out, sample = {}, {}
    points = mr.grid_points(N)
    with mp.Pool(min(8, os.cpu_count() or 1)) as pool:
        for name in MESHES:
            t0 = time.time()
            d = np.load(os.path.join(GOLD, "meshes", name + ".npz"))
            tris = normalised_tris(d["vb"], d["ib"])
            parts = pool.map(_part, [(points[s:s + 1024], tris) for s in range(0, len(points), 1024)])
            d2 = np.concatenate([p[0] for p in parts])
            tri = np.concatenate([p[1] for p in parts])
            out[f"{name}/{N}"] = {"triangles": int(len(tris)), "sample": {"seed": SEED, "voxels": SAMPLE, "file": "mesh_distance_sample.npz"}}
            for b in BANDS:
                out[f"{name}/{N}"][f"band{b}"], sample[f"{name}_band{b}_bits"], sample[f"{name}_band{b}_tri"] = summary(d2, tri, b)
            print(name, len(tris), f"{time.time() - t0:.0f} s", flush=True)
    with open(os.path.join(GOLD, "mesh_distance.json"), "w") as fh:
        json.dump(out, fh, indent=1, sort_keys=True)
        fh.write("\n")
    np.savez_compressed(os.path.join(GOLD, "mesh_distance_sample.npz"), **sample)


if __name__ == "__main__":
    main()
