"""Meshes and made-up records shared by tests/test_edge_centre.py and tests/test_gpu_edge_centre.py: what the lists' edge word
(dxv_dirmap.h: dm_local_entry, dm_ray_local -- cells counted from the texel's centre) is tried on."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

_PINS = np.array([[-1, -1, -1, 0, 0, 1], [1, 1, 1, 0, 0, 1]], np.float32)     # unreferenced vertices: the bound is the cube [-1, 1]^3


def _turn(p, axis, angle):
    c, s = np.cos(angle), np.sin(angle)
    a, b = (axis + 1) % 3, (axis + 2) % 3
    q = p.copy()
    q[:, a], q[:, b] = c * p[:, a] - s * p[:, b], s * p[:, a] + c * p[:, b]
    return q


def octahedron(snap=0):
    """an octahedron of radius 0.7 turned 45 degrees about each axis in turn: eight triangles as large as the faces of the map, none of
    their edges along a texel row -- every texel they cross cuts them with a slanted edge; snap: vertices rounded to multiples of 1 / snap
    (the voxel-centre lattice of a grid of that side: rays through edges and vertices)"""
    p = 0.7 * np.array([[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1]], np.float64)
    for axis in range(3):
        p = _turn(p, axis, np.pi / 4)
    if snap:
        p = np.round(p * snap) / snap
    tris = [(0, 2, 4), (2, 1, 4), (1, 3, 4), (3, 0, 4), (2, 0, 5), (1, 2, 5), (3, 1, 5), (0, 3, 5)]
    pos = np.array([p[list(t)] for t in tris]).reshape(-1, 3)
    nrm = pos / np.linalg.norm(pos, axis=1)[:, None]
    vb = np.hstack([pos, nrm]).astype(np.float32)
    return np.concatenate([vb, _PINS]).astype(np.float32), np.arange(len(pos), dtype=np.uint32)


def meshes(bunny):
    """name -> (vb, ib): the turned octahedron, its lattice-snapped version and the golden bunny"""
    return {"octahedron": octahedron(), "snapped": octahedron(16), "bunny": (bunny[0], bunny[1])}


RECORD = np.dtype([("box", np.float32, 4), ("rr", np.uint32), ("hasTri", np.uint32), ("pad", np.float32), ("px", np.float32, 3),
                   ("py", np.float32, 3), ("pw", np.float32, 3)])
assert RECORD.itemsize == 64


def record(R, i, j, cells_xy, pad_cells=1.5, has_tri=True):
    """a DirRecord whose projected triangle has the vertices `cells_xy` (3 x 2, in cells of texel (i, j): the texel is [0, 128)^2), dilated by
    pad_cells; the footprint box is the dilated triangle's, as the builder's is"""
    per = 1.0 / (64.0 * R)
    u = 2.0 * i / R - 1.0 + np.asarray(cells_xy, np.float64)[:, 0] * per
    v = 2.0 * j / R - 1.0 + np.asarray(cells_xy, np.float64)[:, 1] * per
    pad = pad_cells * per
    rec = np.zeros(1, RECORD)
    lo = lambda x: np.nextafter(np.float32(x), np.float32(-np.inf))
    hi = lambda x: np.nextafter(np.float32(x), np.float32(np.inf))
    rec["box"] = [lo(u.min() - pad), hi(u.max() + pad), lo(v.min() - pad), hi(v.max() + pad)]
    rec["rr"] = 0x3000 | (0x3c00 << 16)
    rec["hasTri"] = 1 if has_tri else 0
    rec["pad"] = pad
    rec["px"], rec["py"], rec["pw"] = u, v, 1.0
    return rec


def records(rng):
    """[(what, R, i, j, record)]: a few thousand (record, texel) pairs"""
    out = []

    def add(what, R, cells_xy, pad=1.5, has_tri=True, at=None):
        i, j = at if at is not None else (int(rng.integers(0, R)), int(rng.integers(0, R)))
        out.append((what, R, i, j, record(R, i, j, cells_xy, pad, has_tri)))

    def through(point, angle, reach=400.0, depth=300.0):
        """a triangle one of whose edges passes through `point` at `angle`, the third vertex `depth` cells to its left"""
        d = np.array([np.cos(angle), np.sin(angle)])
        n = np.array([-d[1], d[0]])
        p = np.asarray(point, np.float64)
        return [p - reach * d, p + reach * d, p + depth * n]

    Rs = (16, 32, 64, 128, 256, 512)
    spots = [(64, 64), (0, 0), (128, 0), (0, 128), (128, 128)]
    for R in Rs:
        corners = [(0, 0), (R - 1, 0), (0, R - 1), (R - 1, R - 1), (R // 2, R // 2)]
        # edges through the texel's centre and through each corner, all round the compass (45 degrees -- |a| = |b| = 127 -- and the axes included)
        for spot in spots:
            for k in range(24):
                add("through %s" % (spot,), R, through(spot, 2 * np.pi * k / 24), at=corners[k % 5])
            for off in (-0.75, -0.25, 0.25, 0.75):
                for k in (1, 3, 5, 7):
                    add("beside %s" % (spot,), R, through((spot[0] + off, spot[1] - off), np.pi * k / 4 + 1e-3 * off))
        # c at both clamp limits: a diagonal edge one cell either side of the corner where a x' + b y' is -16,256, in steps of a sixteenth
        # of a cell -- the constant passes through +-16,256 on the way -- for each of the four diagonals
        for k in (1, 3, 5, 7):
            ang = np.pi * k / 4
            n = np.array([-np.sin(ang), np.cos(ang)])
            far = 64.0 + 64.0 * np.sign(n)                  # the corner the inward normal points at: the edge beyond it cuts the whole texel
            near = 64.0 - 64.0 * np.sign(n)                 # ... and beyond this one, nothing
            for corner in (far, near):
                for step in range(-24, 25):
                    add("clamp", R, through(corner + n * step / 16.0 * np.sqrt(0.5), ang))
        # axis-parallel edges at cell borders and inside cells
        for x in (0.0, 0.5, 1.0, 63.5, 64.0, 127.0, 127.5, 128.0):
            add("axis", R, [(x, -300), (x, 300), (x + 200, 0)])
            add("axis", R, [(x, 300), (x, -300), (x - 200, 0)])
            add("axis", R, [(-300, x), (300, x), (0, x - 200)])
            add("axis", R, [(300, x), (-300, x), (0, x + 200)])
        # slivers: long, a fraction of a cell wide, through the texel at random
        for _ in range(40):
            p, ang = rng.uniform(0, 128, 2), rng.uniform(0, 2 * np.pi)
            d = np.array([np.cos(ang), np.sin(ang)])
            n = np.array([-d[1], d[0]])
            add("sliver", R, [p - 500 * d, p + 500 * d, p + n * 10.0 ** rng.uniform(-6, 0)], pad=rng.uniform(0.05, 3.0))
        # small and large random triangles, either winding
        for _ in range(80):
            c, s = rng.uniform(-20, 148, 2), 10.0 ** rng.uniform(0, 3)
            add("random", R, c + rng.uniform(-s, s, (3, 2)), pad=rng.uniform(0.05, 3.0))
        # no projected triangle: the box alone
        for _ in range(4):
            add("no triangle", R, rng.uniform(0, 128, (3, 2)), has_tri=False)
    return out
