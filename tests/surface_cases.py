"""Hostile triangles for the surface rule's candidate enumerations (csrc/dxv_surface.h), shared by tests/test_surface_walk.py and
tests/test_gpu_surface_walk.py.  Test helper, not collected.

Every generator is deterministic (fixed seeds) and returns float32 triangles (K, 3 vertices, 3) in the scene's NORMALISED coordinates
(the grid is [-1, 1]^3, y flipped, voxel i spans [i, i + 1] * 2 / N - 1) for the grid side N it is given.  `families(N)` is the whole
set, `picked(N)` the first PICK of each family -- what the GPU module runs one triangle per launch."""
import numpy as np

import surface_restated as sr

F = np.float32
PICK = 20
BANDS = ((0.5, 2.0), (2.0, 3.5), (3.5, 4.75), (4.75, 6.0))           # log10 of a far vertex's magnitude

# triangles a numpy mirror of the column walk (before far triangles were given their whole box) lost voxels of: (N, triangle)
LISTED = [
    (64, [[-705516.0, 824350.5625, -568098.4375], [-27069.623046875, -7590.45361328125, -1112.255126953125], [0.7736790776252747, -0.7238471508026123, -0.1894415020942688]]),
    (64, [[-0.8033004999160767, 0.8040252327919006, 0.612873375415802], [-2485.70263671875, -403890.4375, -848220.25], [-231.98001098632812, 74756.0234375, 342.6063232421875]]),
    (64, [[77529.9453125, 479737.15625, 734549.1875], [0.6010757684707642, -0.40475231409072876, 0.8606647849082947], [-0.9002138376235962, -0.26541751623153687, 0.17929358780384064]]),
    (64, [[-541038.1875, 865382.875, 272654.15625], [-112810.765625, -40894.6640625, 208018.375], [0.8837296962738037, -0.684445321559906, 0.03545796498656273]]),
    (32, [[-884365.1875, 288075.25, -624139.6875], [-0.6483529210090637, -0.22502575814723969, 0.4410402178764343], [-0.9291523098945618, 0.9950888156890869, -0.44348132610321045]]),
    (32, [[222608.875, -465986.875, 937648.5], [331147.6875, 260778.5, -166352.125], [-0.3730601668357849, -0.28452882170677185, -0.6948755979537964]]),
]


def listed(N=None):
    return np.asarray([t for n, t in LISTED if N is None or n == N], F).reshape(-1, 3, 3)


def face(N, i):
    """the plane between voxels i - 1 and i along x or z (exact for a power-of-two N); along y it is the negation of a face"""
    return F(sr.centres(N, i)) - F(1) / F(N)


def at(N, u):
    """the normalised x / z coordinate of voxel-unit position u (the y coordinate is its negation), float32"""
    return F(F(u) / F(N) * F(2) - F(1))


def _axes(k, w, u, v):
    """a point with coordinate w on axis k and (u, v) on the two axes after it"""
    p = [F(0)] * 3
    p[k], p[(k + 1) % 3], p[(k + 2) % 3] = w, u, v
    return p


def on_face(N):
    """planes lying exactly on a voxel face and one float32 ulp to either side, 6 x 6 voxels wide: the box holds 2 x 7 x 7 voxels"""
    out = []
    for k in range(3):
        for i in (N // 2, 3, N - 2):
            f = face(N, i)
            lo = 2 + (i + k) % 3
            a, b = at(N, lo + 0.3), at(N, lo + 6.6)
            for w in (np.nextafter(f, F(-2)), f, np.nextafter(f, F(2))):
                out.append([_axes(k, w, a, a), _axes(k, w, b, a), _axes(k, w, a, b)])
    return np.asarray(out, F)


def box_64_65(N):
    """one right triangle inside a single layer of voxels, its legs scaled so that the box holds exactly 64 (1 x 8 x 8, 1 x 4 x 16)
    and exactly 65 (1 x 5 x 13, 1 x 13 x 5) voxels; and a tilted one in 4 x 4 x 4"""
    out = []
    for k in range(3):
        w = at(N, 5.5)
        for eu, ev in ((8, 8), (4, 16), (5, 13), (13, 5)):
            u0, v0 = 1.25, 2.25 if ev < 14 else 0.25
            out.append([_axes(k, w, at(N, u0), at(N, v0)), _axes(k, w, at(N, u0 + eu - 0.5), at(N, v0)), _axes(k, w, at(N, u0), at(N, v0 + ev - 0.5))])
        out.append([_axes(k, at(N, 4.25), at(N, 3.25), at(N, 2.25)), _axes(k, at(N, 7.75), at(N, 6.75), at(N, 3.0)), _axes(k, at(N, 5.0), at(N, 4.0), at(N, 5.75))])
    out = np.asarray(out, F)
    for t, want in zip(out, [64, 64, 65, 65, 64] * 3):
        lo, hi = sr.kernel_box(t, N)
        assert np.prod(np.asarray(hi) - np.asarray(lo) + 1) == want, (t, lo, hi)
    return out


def slivers(N, count=24):
    """triangles across the whole grid whose third vertex is 10^-7 to 10^-2 beside the long edge"""
    rng = np.random.default_rng(7100 + N)
    out = []
    for i, width in enumerate(np.tile(10.0 ** np.linspace(-7, -2, 6), count // 6)):
        a = rng.uniform(-1.05, -0.6, 3) * rng.choice([-1, 1], 3)
        b = -a + rng.uniform(-0.3, 0.3, 3)
        d = np.cross(b - a, rng.normal(size=3))
        d = (a + b) * rng.uniform(0.1, 0.9) + width * d / np.linalg.norm(d) if i % 2 else b + width * d / np.linalg.norm(d)
        out.append([a, b, d])
    return np.asarray(out, F)


def degenerates(N):
    """exact degenerates: two equal vertices, three collinear vertices (dyadic coordinates: collinear in float32 as well), a segment
    along each axis through voxel centres, a segment along a voxel edge -- as long as the grid allows"""
    out = []
    lo, hi, mid = at(N, 1.25), at(N, N - 1.25), at(N, N // 2 + 0.5)
    for k in range(3):
        p, q = _axes(k, lo, lo, hi), _axes(k, hi, hi, lo)
        out += [[p, q, q], [p, p, q]]                                        # two equal vertices, on a diagonal
        a, b = np.asarray(_axes(k, F(-0.75), F(-0.5), F(0.25)), F), np.asarray(_axes(k, F(0.75), F(0.5), F(-0.5)), F)
        out.append([a, (a + b) / F(2), b])                                   # three collinear vertices
        out.append([a, b, (a + b) / F(2) + (b - a) / F(8)])
        out.append([_axes(k, lo, mid, mid), _axes(k, hi, mid, mid), _axes(k, hi, mid, mid)])            # along the axis, through centres
        out.append([_axes(k, lo, mid, mid), _axes(k, at(N, 3.5), mid, mid), _axes(k, hi, mid, mid)])
        e, g = face(N, N // 2), face(N, 3)
        out.append([_axes(k, lo, e, g), _axes(k, hi, e, g), _axes(k, hi, e, g)])                        # along a voxel edge: 2 x 2 x L
        out.append([_axes(k, lo, e, g), _axes(k, at(N, 7.0), e, g), _axes(k, hi, e, g)])
    out.append([[F(0.1), F(0.2), F(-0.3)]] * 3)                              # a point
    return np.asarray(out, F)


def ties(N):
    """dominant-axis ties: planes with normals (1, 1, 1), (1, 1, 0), (1, -1, 0) and their permutations, vertices on dyadic coordinates
    (the cross product ties exactly); through a voxel corner and through a generic point"""
    normals = [(1, 1, 1), (1, 1, -1), (1, -1, 1), (-1, 1, 1), (1, 1, 0), (1, 0, 1), (0, 1, 1), (1, -1, 0), (1, 0, -1), (0, 1, -1)]
    out = []
    for n in normals:
        n = np.asarray(n, np.int64)
        e = np.eye(3, dtype=np.int64)[int(np.argmin(np.abs(n)))] if 0 in n else np.asarray([1, -1, 0]) * np.asarray([1, n[0] * n[1], 1])
        u = np.cross(n, e) if 0 in n else e
        v = np.cross(n, u)
        assert n @ u == 0 and n @ v == 0 and np.abs(np.cross(u, v)).max() > 0
        for p0, s in ((np.asarray([-0.25, 0.125, 0.0]), 0.375), (np.asarray([0.046875, -0.203125, 0.109375]), 0.21875)):
            out.append([p0 - s * u - s * v / 2, p0 + s * u, p0 + s * v])
    out = np.asarray(out, np.float64)
    assert np.array_equal(out.astype(F).astype(np.float64), out)
    return out.astype(F)


def leaving(N):
    """triangles that leave the grid on each of the six sides, and triangles just outside each side: one float32 ulp beyond it, and
    exactly on it (the closed boxes of the outermost layer touch that one)"""
    rng = np.random.default_rng(7300 + N)
    out = []
    for k in range(3):
        for side in (-1, 1):
            for _ in range(2):
                t = rng.uniform(-0.8, 0.8, (3, 3))
                t[rng.integers(3), k] = side * rng.uniform(1.05, 1.9)
                t[rng.integers(3), k] = side * rng.uniform(0.2, 1.5)
                out.append(t)
            for w in (np.nextafter(F(1), F(2)), F(1)):
                t = rng.uniform(-0.9, 0.9, (3, 3))
                t[:, k] = side * (float(w) + np.asarray([0.0, 0.0, 0.3]) * (w > 1))
                out.append(t)
    return np.asarray(out, F)


def far(N, per_band=10, seed=7400):
    """one vertex (even index) or two (odd) of magnitude 10^0.5 to 10^6, in four bands, the others inside [-1.2, 1.2]^3"""
    rng = np.random.default_rng(seed + N)
    out = []
    for lo, hi in BANDS:
        for i in range(per_band):
            t = rng.uniform(-1.2, 1.2, (3, 3))
            for v in rng.permutation(3)[: 1 + i % 2]:
                t[v] = 10.0 ** rng.uniform(lo, hi) * rng.uniform(-1, 1, 3)
            out.append(t)
    return np.asarray(out, F)


def top_band(N, count, seed=7500):
    """far triangles of the highest band only"""
    return far(N, count, seed)[-count:]


def families(N):
    return {"on_face": on_face(N), "box_64_65": box_64_65(N), "slivers": slivers(N), "degenerates": degenerates(N), "ties": ties(N),
            "leaving": leaving(N), "far": np.concatenate([far(N), listed()])}


def picked(N):
    """about PICK triangles of each family (spread over the family, the listed far ones always among them)"""
    out = {}
    for name, t in families(N).items():
        idx = np.unique(np.linspace(0, len(t) - 1, min(PICK, len(t))).round().astype(int))
        if name == "far":
            idx = np.unique(np.r_[idx, np.arange(len(t) - len(LISTED), len(t))])
        out[name] = t[idx]
    return out


def shares(N, world, zblock):
    """(rank, the global slices of its block-cyclic share: blocks of zblock slices dealt round robin), ranks that get none left out"""
    for rank in range(world):
        z = np.asarray([z for z in range(N) if (z // zblock) % world == rank], np.int64)
        if len(z):
            yield rank, z
