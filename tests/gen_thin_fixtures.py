"""Makes tests/golden/thin.json: both kinds of dxv_thin on the filled conservative surface of the bunny at 256^3 (DXV_MODE_SURFACE, then
DXV_FILL_SOLID), too large for a test to restate quickly.  CPU only, not part of the suite:

    python tests/gen_thin_fixtures.py

The surface grid comes from the numpy restatement (tests/surface_restated.py) and its hash is asserted against tests/golden/fill.json, the
fill from tests/fill_restated.py, the thinning from tests/thin_restated.py.  Recorded: the input's solid count and the SHA-256 of its grid
packed to a bit per voxel (thin_restated.packed_sha), and per kind the solid count, that hash, the iterations and the voxels removed."""
import hashlib
import json
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.join(HERE, "golden")
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

import fill_restated as fr  # noqa: E402
import surface_restated as sr  # noqa: E402
import thin_restated as tr  # noqa: E402

SIDE = 256


def main():
    d = np.load(os.path.join(GOLD, "meshes", "bunny.npz"))
    surface = sr.surface_of_mesh(d["vb"], d["ib"], SIDE)
    with open(os.path.join(GOLD, "fill.json")) as fh:
        assert hashlib.sha256(np.ascontiguousarray(surface).tobytes()).hexdigest() == json.load(fh)[f"bunny/{SIDE}"]["grid_sha256"]
    grid = fr.fill(surface)
    out = {"side": SIDE, "grid_count": int(np.count_nonzero(grid)), "grid_packed_sha256": tr.packed_sha(grid)}
    for kind, tag in zip(tr.KINDS, ("curve", "kernel")):
        t0 = time.time()
        after, iterations, removed, converged = tr.thin(grid, kind)
        count = int(np.count_nonzero(after))
        assert converged and 0 < count < out["grid_count"] and removed == out["grid_count"] - count
        out[tag] = {"count": count, "iterations": iterations, "removed": removed, "packed_sha256": tr.packed_sha(after)}
        print(tag, out[tag], f"{time.time() - t0:.1f} s")
    with open(os.path.join(GOLD, "thin.json"), "w") as fh:
        json.dump({f"bunny/{SIDE}": out}, fh, indent=1, sort_keys=True)
        fh.write("\n")


if __name__ == "__main__":
    main()
