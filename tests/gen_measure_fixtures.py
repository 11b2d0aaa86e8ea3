"""Makes tests/golden/measure.json: the measures (dxv_measure) of grids too large for a test to restate quickly.  CPU only:

    python tests/gen_measure_fixtures.py

The grids (DXV_MODE_REFERENCE) are the CPU oracle's (oracle/orc.py), the ones tests/gen_components_fixtures.py labels: their SHA-256 must
equal the one tests/golden/components.json records.  Labelling and measures are the restatement's (tests/measure_restated.py, with scipy's
labelling numbered by first voxel); at 64^3 (bunny) they are first asserted equal, as bytes, to the measures of components_restated.label's
own labelling.  Recorded per configuration: the grid's hash, and for SOLID 26 and EMPTY 6 K, record 0 in full and the hash of the table."""
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

import components_restated as cr  # noqa: E402
import measure_restated as ms  # noqa: E402
from gen_components_fixtures import CONFIGS, mesh, sha  # noqa: E402

CASES = ((cr.SOLID, 26, "solid/26"), (cr.EMPTY, 6, "empty/6"))


def main():
    from oracle import orc
    with open(os.path.join(GOLD, "components.json")) as fh:
        known = json.load(fh)
    out = {}
    for name, N in [("bunny", 64)] + CONFIGS:
        t0 = time.time()
        vb, ib = mesh(name)
        grid = orc.Scene(vb, ib).voxelize(N)
        key = f"{name}/{N}"
        row = {"grid_sha256": sha(grid)}
        if key in known:
            assert row["grid_sha256"] == known[key]["grid_sha256"], f"{key}: the oracle's grid differs from the one the components' fixture was made from"
        for of, conn, tag in CASES:
            table = ms.measure(grid, of, conn)
            if N == 64:
                assert table.tobytes() == ms.measure(grid, of, conn, cr.label(grid, of, conn)).tobytes(), f"{key} {tag}: scipy's labelling differs from the restatement's"
            if key in known:
                assert len(table) - 1 == known[key][tag]["count"], (key, tag)
            row[tag] = {"count": len(table) - 1, "record0": {n: np.asarray(table[0][n]).tolist() for n in ms.RECORD.names}, "table_sha256": sha(table)}
        if N != 64:
            out[key] = row
        print(key, row, f"{time.time() - t0:.0f} s", flush=True)
    with open(os.path.join(GOLD, "measure.json"), "w") as fh:
        json.dump(out, fh, indent=1, sort_keys=True)
        fh.write("\n")


if __name__ == "__main__":
    main()
