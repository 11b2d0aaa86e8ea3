"""Makes tests/golden/surface.json: the surface rule (DXV_MODE_SURFACE) and the solid with its shell (DXV_MODE_REFERENCE_SURFACE) for
configurations too large for a test to restate quickly.  CPU only:

    python tests/gen_surface_fixtures.py

The surface comes from the numpy restatement (tests/surface_restated.py), in float32 and, as a cross-check, in float64 (the number of
voxels where the two differ is recorded).  The solid part of mode 3 comes from the CPU oracle (oracle/orc.py); its SHA-256 is checked
against tests/golden/grids.json and configs.json where they have one.  Hashes are over the whole uint8 [z, y, x] grid."""
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

import surface_restated as sr  # noqa: E402
from dxrvoxelizer_amd import meshes  # noqa: E402

CONFIGS = [("torus1m", 512), ("dragon9", 512), ("cube", 1024), ("tetrahedron", 1024)]


def mesh(name):
    if name == "torus1m":
        return meshes.torus()
    if name == "dragon9":
        d = np.load(os.path.join(GOLD, "meshes", "dragon.npz"))
        return meshes.trisect(d["vb"], d["ib"])
    return getattr(meshes, name)()


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def main():
    from oracle import orc
    known = {}
    for fn in ("grids.json", "configs.json"):
        with open(os.path.join(GOLD, fn)) as fh:
            known.update({k: v["sha256"] for k, v in json.load(fh).items()})
    out = {}
    for name, N in CONFIGS:
        t0 = time.time()
        vb, ib = mesh(name)
        tris = sr.normalised_tris(vb, ib)
        surf = sr.surface_grid(tris, N)
        diff = int(np.count_nonzero(surf != sr.surface_grid(tris, N, np.float64)))
        solid = orc.Scene(vb, ib).voxelize(N)
        key = f"{name}/{N}/reference"
        if key in known:
            assert sha(solid) == known[key], f"{key}: the oracle's solid differs from the committed fixture"
        shell = solid | surf
        out[f"{name}/{N}"] = {
            "tris": int(len(tris)),
            "surface": {"sha256": sha(surf), "count": int(np.count_nonzero(surf))},
            "reference_surface": {"sha256": sha(shell), "count": int(np.count_nonzero(shell))},
            "solid": {"sha256": sha(solid), "count": int(np.count_nonzero(solid)), "checked_against": key if key in known else None},
            "f32_f64_differences": diff,
        }
        print(name, N, out[f"{name}/{N}"], f"{time.time() - t0:.0f} s", flush=True)
        del surf, solid, shell
    with open(os.path.join(GOLD, "surface.json"), "w") as fh:
        json.dump(out, fh, indent=1, sort_keys=True)
        fh.write("\n")


if __name__ == "__main__":
    main()
