"""Makes tests/golden/fill.json: the exterior flood fill (dxv_fill, both kinds) of surface grids too large for a test to restate
quickly.  CPU only:

    python tests/gen_fill_fixtures.py

The surface grids (DXV_MODE_SURFACE) come from the numpy restatement (tests/surface_restated.py); their SHA-256 is asserted against
tests/golden/surface.json where that file has the configuration.  The fill comes from scipy.ndimage.label where scipy is present
(default structure = 6-connectivity; outside = the components of the free space that touch the grid's border), otherwise from the
restatement (tests/fill_restated.py); at 64^3 and 128^3 (bunny) scipy's result is first asserted equal to the restatement.  Recorded
per configuration: the grid's hash and count, the result's hash and count per kind, and what it was made with.  The tetrahedron at
1024^3 is left out: its labelling (a 4 GiB label array beside the grid and its masks) does not fit in memory on a CPU box of the kind
the other fixtures were made on; the cube at 1024^3 needs no fixture (tests/test_gpu_fill.py: its shell lies on the grid's border)."""
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

import fill_restated as fr  # noqa: E402
import surface_restated as sr  # noqa: E402
from dxrvoxelizer_amd import meshes  # noqa: E402

CONFIGS = [("bunny", 256), ("torus1m", 512), ("dragon9", 512)]


def mesh(name):
    if name == "torus1m":
        return meshes.torus()
    d = np.load(os.path.join(GOLD, "meshes", ("dragon" if name == "dragon9" else name) + ".npz"))
    return meshes.trisect(d["vb"], d["ib"]) if name == "dragon9" else (d["vb"], d["ib"])


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def scipy_outside(grid):
    """the outside set through scipy.ndimage.label, or None without scipy"""
    try:
        from scipy import ndimage
    except ImportError:
        return None
    labels, n = ndimage.label(grid == 0)
    touches = np.zeros(n + 1, bool)
    for axis in range(3):
        for side in (0, -1):
            idx = [slice(None)] * 3
            idx[axis] = side
            touches[np.unique(labels[tuple(idx)])] = True
    touches[0] = False
    return touches[labels]


def outside(grid):
    out = scipy_outside(grid)
    return fr.outside(grid) if out is None else out


def main():
    with open(os.path.join(GOLD, "surface.json")) as fh:
        known = json.load(fh)
    with_scipy = scipy_outside(np.zeros((2, 2, 2), np.uint8)) is not None
    vb, ib = mesh("bunny")
    for N in (64, 128):
        g = sr.surface_of_mesh(vb, ib, N)
        assert np.array_equal(outside(g), fr.outside(g)), f"bunny {N}: scipy's labelling differs from the restatement"
    out = {}
    for name, N in CONFIGS:
        t0 = time.time()
        vb, ib = mesh(name)
        grid = sr.surface_of_mesh(vb, ib, N)
        key = f"{name}/{N}"
        if key in known:
            assert sha(grid) == known[key]["surface"]["sha256"], f"{key}: the restated surface differs from the committed fixture"
        o = outside(grid)
        row = {"grid_sha256": sha(grid), "grid_count": int(np.count_nonzero(grid)), "checked_against": f"surface.json {key}" if key in known else None,
               "made_with": "scipy" if with_scipy else "restatement"}
        for what, tag in ((fr.SOLID, "solid"), (fr.INTERIOR, "interior")):
            f = fr.fill_from(grid, o, what)
            row[tag] = {"sha256": sha(f), "count": int(np.count_nonzero(f))}
        out[key] = row
        print(key, row, f"{time.time() - t0:.0f} s", flush=True)
        del grid, o
    with open(os.path.join(GOLD, "fill.json"), "w") as fh:
        json.dump(out, fh, indent=1, sort_keys=True)
        fh.write("\n")


if __name__ == "__main__":
    main()
