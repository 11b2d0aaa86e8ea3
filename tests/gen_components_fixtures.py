"""Makes tests/golden/components.json: the connected components (dxv_components, both kinds, both connectivities) of grids too large for a
test to restate quickly.  CPU only:

    python tests/gen_components_fixtures.py

The grids (DXV_MODE_REFERENCE) are the CPU oracle's (oracle/orc.py), as in tests/gen_distance_fixtures.py; their SHA-256 must equal the
committed fixture's (tests/golden/grids.json) where that file has the configuration.  The labelling comes from
scipy.ndimage.label with generate_binary_structure(3, 1) and (3, 3) -- its numbering is the rule's: components in the order of their first
voxel in C order --, the table from bincount and find_objects.  At 64^3 (bunny, both kinds, both connectivities) scipy's labels and the
table made here are first asserted equal to the restatement (tests/components_restated.py).  Recorded per configuration: the grid's hash,
and per kind and connectivity K and the hashes of labels (uint32) and table (24-byte records)."""
import hashlib
import json
import os
import sys
import time

import numpy as np
from scipy import ndimage

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
GOLD = os.path.join(HERE, "golden")
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)

import components_restated as cr  # noqa: E402
from dxrvoxelizer_amd import meshes  # noqa: E402

CONFIGS = [("bunny", 256), ("torus1m", 512)]


def mesh(name):
    if name == "torus1m":
        vb, ib = meshes.torus()
    else:
        d = np.load(os.path.join(GOLD, "meshes", name + ".npz"))
        vb, ib = d["vb"], d["ib"]
    return np.ascontiguousarray(vb, np.float32).reshape(-1, 6), np.ascontiguousarray(ib, np.uint32)


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def scipy_label(grid, of, connectivity):
    """(labels uint32, table) through scipy"""
    N = grid.shape[0]
    want, K = ndimage.label(cr.members(grid, of), structure=ndimage.generate_binary_structure(3, 1 if connectivity == 6 else 3))
    labels = want.astype(np.uint32)
    table = np.zeros(K, cr.RECORD)
    if K:
        flat = want.ravel()
        table["voxels"] = np.bincount(flat, minlength=K + 1)[1:]
        values, where = np.unique(flat, return_index=True)
        table["first"] = where[values > 0]
        for k, box in enumerate(ndimage.find_objects(want)):
            z, y, x = box
            table["lo"][k] = (x.start, y.start, z.start)
            table["hi"][k] = (x.stop - 1, y.stop - 1, z.stop - 1)
        table["flags"] = ((table["lo"] == 0) | (table["hi"] == N - 1)).any(axis=1)
    return labels, table


def main():
    from oracle import orc
    with open(os.path.join(GOLD, "grids.json")) as fh:
        known = json.load(fh)
    out = {}
    for name, N in [("bunny", 64)] + CONFIGS:
        t0 = time.time()
        vb, ib = mesh(name)
        grid = orc.Scene(vb, ib).voxelize(N)
        key = f"{name}/{N}"
        if f"{key}/reference" in known:
            assert sha(grid) == known[f"{key}/reference"]["sha256"], f"{key}: the oracle's grid differs from the committed fixture"
        row = {"grid_sha256": sha(grid), "grid_count": int(np.count_nonzero(grid)), "checked_against": f"grids.json {key}/reference" if f"{key}/reference" in known else None}
        for of, kind in ((cr.SOLID, "solid"), (cr.EMPTY, "empty")):
            for conn in (6, 26):
                labels, table = scipy_label(grid, of, conn)
                if N == 64:
                    want, wtable = cr.label(grid, of, conn)
                    assert np.array_equal(labels, want) and np.array_equal(table, wtable), f"{key} {kind} {conn}: scipy differs from the restatement"
                row[f"{kind}/{conn}"] = {"count": len(table), "labels_sha256": sha(labels), "table_sha256": sha(table)}
        if N != 64:
            out[key] = row
        print(key, row, f"{time.time() - t0:.0f} s", flush=True)
    with open(os.path.join(GOLD, "components.json"), "w") as fh:
        json.dump(out, fh, indent=1, sort_keys=True)
        fh.write("\n")


if __name__ == "__main__":
    main()
