"""Makes tests/golden/distance.json: the signed distance field (DXV_DIST_SQ_I32) of grids too large for a test to restate quickly.
CPU only:

    python tests/gen_distance_fixtures.py

The grid is the CPU oracle's (oracle/orc.py); its SHA-256 must equal the committed fixture's (tests/golden/grids.json, configs.json).
The field is the numpy restatement's (tests/distance_restated.py) -- or, where scipy is present, scipy.ndimage's exact Euclidean
transform (nearest-voxel indices, squared in integers), which is first asserted equal to the restatement on the bunny at 64^3 and
128^3.  Recorded per configuration: the grid's hash the field was made from, the SHA-256 of the int32 [z, y, x] field, its min, max
and sum.  1024^3 (a 4 GiB field, 8 G voxel indices in scipy) is left out: its generation does not stay within minutes on a CPU box."""
import hashlib
import json
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
GOLD = os.path.join(HERE, "golden")
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)

import distance_restated as dr  # noqa: E402
from dxrvoxelizer_amd import meshes  # noqa: E402

CONFIGS = [("bunny", 256), ("torus1m", 512), ("dragon9", 512)]


def mesh(name):
    if name == "torus1m":
        return meshes.torus()
    d = np.load(os.path.join(GOLD, "meshes", ("dragon" if name == "dragon9" else name) + ".npz"))
    return meshes.trisect(d["vb"], d["ib"]) if name == "dragon9" else (d["vb"], d["ib"])


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def scipy_field(grid):
    """DXV_DIST_SQ_I32 through scipy.ndimage.distance_transform_edt's nearest-voxel indices, or None without scipy"""
    try:
        from scipy import ndimage
    except ImportError:
        return None
    solid = grid != 0
    out = np.empty(grid.shape, np.int32)
    for feature, mine, sign in ((solid, ~solid, 1), (~solid, solid, -1)):       # empty voxels look for solid ones, and the reverse
        if not mine.any():
            continue
        if not feature.any():
            out[mine] = sign * dr.NONE
            continue
        idx = ndimage.distance_transform_edt(~feature, return_distances=False, return_indices=True)
        d2 = np.zeros(grid.shape, np.int32)
        for axis in range(3):
            shape = [1, 1, 1]
            shape[axis] = grid.shape[axis]
            d2 += (idx[axis] - np.arange(grid.shape[axis], dtype=np.int32).reshape(shape)) ** 2
        del idx
        out[mine] = sign * d2[mine]
    return out


def field(grid):
    f = scipy_field(grid)
    return dr.distance_sq(grid) if f is None else f


def main():
    from oracle import orc
    known = {}
    for fn in ("grids.json", "configs.json"):
        with open(os.path.join(GOLD, fn)) as fh:
            known.update({k: v["sha256"] for k, v in json.load(fh).items()})
    vb, ib = mesh("bunny")
    for N in (64, 128):
        g = orc.Scene(vb, ib).voxelize(N)
        assert np.array_equal(field(g), dr.distance_sq(g)), f"bunny {N}: scipy's field differs from the restatement"
    out = {}
    for name, N in CONFIGS:
        t0 = time.time()
        vb, ib = mesh(name)
        grid = orc.Scene(vb, ib).voxelize(N)
        key = f"{name}/{N}/reference"
        assert sha(grid) == known[key], f"{key}: the oracle's grid differs from the committed fixture"
        f = field(grid)
        out[f"{name}/{N}"] = {"grid_sha256": sha(grid), "sha256": sha(f), "min": int(f.min()), "max": int(f.max()),
                              "sum": int(f.sum(dtype=np.int64)), "made_with": "restatement" if scipy_field(grid[:2, :2, :2]) is None else "scipy"}
        print(name, N, out[f"{name}/{N}"], f"{time.time() - t0:.0f} s", flush=True)
        del grid, f
    with open(os.path.join(GOLD, "distance.json"), "w") as fh:
        json.dump(out, fh, indent=1, sort_keys=True)
        fh.write("\n")


if __name__ == "__main__":
    main()
