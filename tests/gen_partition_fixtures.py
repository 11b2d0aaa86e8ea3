"""Makes tests/golden/partition_hashes.json: the maximal-ball partition (dxv_partition) of the committed 64^3 bunny grid (tests/golden/grids64.npz,
bunny_64_reference) for solid / 65, empty / 65 and solid / 1025 -- SHA-256 of the labels (uint32 [64, 64, 64]), of the table (32-byte records) and
of the throats (20-byte records), with K, T and the interface faces.  CPU only:

    python tests/gen_partition_fixtures.py

Everything is the numpy restatement's (tests/partition_restated.py, form (a)), never the product's."""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.join(HERE, "golden")
sys.path.insert(0, HERE)

import partition_restated as pr  # noqa: E402

CASES = (("solid", pr.SOLID, 65), ("empty", pr.EMPTY, 65), ("solid", pr.SOLID, 1025))


def bunny_grid():
    return np.unpackbits(np.load(os.path.join(GOLD, "grids64.npz"))["bunny_64_reference"])[: 64 ** 3].reshape(64, 64, 64).astype(np.uint8)


def main():
    grid = bunny_grid()
    out = {"grid_sha256": pr.sha(grid)}
    for tag, of, cap in CASES:
        labels, table, throats = pr.partition(grid, of, cap)
        out[f"{tag}/{cap}"] = {"labels_sha256": pr.sha(labels), "table_sha256": pr.sha(table), "throats_sha256": pr.sha(throats), "regions": len(table), "throats": len(throats),
                               "interface_faces": int(throats["faces"].sum()), "largest_radius_sq": int(table["radius_sq"].max())}
        print(tag, cap, out[f"{tag}/{cap}"], flush=True)
    with open(os.path.join(GOLD, "partition_hashes.json"), "w") as fh:
        json.dump(out, fh, indent=1, sort_keys=True)
        fh.write("\n")


if __name__ == "__main__":
    main()
