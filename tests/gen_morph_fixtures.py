"""Makes tests/golden/morph.json: the four operations of dxv_morph at radius_sq = 9 on the bunny's surface grid at 256^3 (DXV_MODE_SURFACE),
too large for a test to restate quickly.  CPU only, not part of the suite:

    python tests/gen_morph_fixtures.py

The surface grid comes from the numpy restatement (tests/surface_restated.py) and its hash is asserted against tests/golden/fill.json; the
morphs come from the shift restatement (tests/morph_restated.py).  Recorded: solid counts, voxels set and cleared, and the SHA-256 of the
grids packed to a bit per voxel (morph_restated.packed_sha).  That shell erodes to nothing at radius_sq 9, so a second entry holds ERODE
and OPEN of the shell dilated by radius_sq 16 first."""
import hashlib
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.join(HERE, "golden")
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

import morph_restated as mr  # noqa: E402
import surface_restated as sr  # noqa: E402

RADIUS_SQ = 9
THICKEN = 16


def main():
    d = np.load(os.path.join(GOLD, "meshes", "bunny.npz"))
    grid = sr.surface_of_mesh(d["vb"], d["ib"], 256)
    with open(os.path.join(GOLD, "fill.json")) as fh:
        assert hashlib.sha256(np.ascontiguousarray(grid).tobytes()).hexdigest() == json.load(fh)["bunny/256"]["grid_sha256"]
    out = {"radius_sq": RADIUS_SQ, "grid_count": int(np.count_nonzero(grid)), "grid_packed_sha256": mr.packed_sha(grid)}
    for op, tag in zip(mr.OPS, ("dilate", "erode", "open", "close")):
        after = mr.morph(grid, op, RADIUS_SQ)
        was_set, cleared = mr.counts(grid, after)
        out[tag] = {"count": int(np.count_nonzero(after)), "set": was_set, "cleared": cleared, "packed_sha256": mr.packed_sha(after)}
        print(tag, out[tag])
    # the shell erodes to nothing at this radius: dilated by THICKEN first, ERODE and OPEN leave something to compare
    thick = mr.morph(grid, mr.DILATE, THICKEN)
    fat = {"radius_sq": RADIUS_SQ, "thickened_by_radius_sq": THICKEN, "grid_count": int(np.count_nonzero(thick)), "grid_packed_sha256": mr.packed_sha(thick)}
    for op, tag in ((mr.ERODE, "erode"), (mr.OPEN, "open")):
        after = mr.morph(thick, op, RADIUS_SQ)
        was_set, cleared = mr.counts(thick, after)
        fat[tag] = {"count": int(np.count_nonzero(after)), "set": was_set, "cleared": cleared, "packed_sha256": mr.packed_sha(after)}
        print("thick", tag, fat[tag])
    with open(os.path.join(GOLD, "morph.json"), "w") as fh:
        json.dump({"bunny/256": out, "bunny/256 thick": fat}, fh, indent=1, sort_keys=True)
        fh.write("\n")


if __name__ == "__main__":
    main()
