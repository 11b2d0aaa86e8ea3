"""Makes tests/golden/thickness.json: the local thickness (dxv_thickness) of the committed 64^3 bunny grid (tests/golden/grids64.npz,
bunny_64_reference) for both kinds at cap_sq 65 and 4096 -- SHA-256 of the map (uint32 [64, 64, 64]) and of the histogram (uint64 [cap_sq + 1]),
the largest value and the minimum wall.  CPU only:

    python tests/gen_thickness_fixtures.py

Map and histogram are the host library's (tests/thickness_host.py: the product's routines run serially), which tests/test_thickness_rule.py
holds to the numpy restatement; at cap_sq 65 the restatement itself is asserted equal here."""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.join(HERE, "golden")
sys.path.insert(0, HERE)

import thickness_host as th  # noqa: E402
import thickness_restated as tr  # noqa: E402

CAPS = (65, 4096)


def bunny_grid():
    return np.unpackbits(np.load(os.path.join(GOLD, "grids64.npz"))["bunny_64_reference"])[: 64 ** 3].reshape(64, 64, 64).astype(np.uint8)


def main():
    grid = bunny_grid()
    out = {"grid_sha256": tr.sha(grid)}
    for of, tag in ((tr.SOLID, "solid"), (tr.EMPTY, "empty")):
        for cap in CAPS:
            W, hist, (centres, items) = th.thickness(grid, of, cap)
            if cap == 65:
                assert W.tobytes() == tr.thickness(grid, of, cap).tobytes(), (tag, cap)
            assert hist.tobytes() == tr.histogram(W, cap).tobytes()
            above = np.flatnonzero(hist[1:])
            out[f"{tag}/{cap}"] = {"field_sha256": tr.sha(W), "histogram_sha256": tr.sha(hist), "max": int(W.max()), "minimum_wall": int(above[0]) + 1 if len(above) else 0,
                                   "centres_painted": centres, "work_items": items}
            print(tag, cap, out[f"{tag}/{cap}"], flush=True)
    with open(os.path.join(GOLD, "thickness.json"), "w") as fh:
        json.dump(out, fh, indent=1, sort_keys=True)
        fh.write("\n")


if __name__ == "__main__":
    main()
