"""An independent numpy restatement of the mesh distance rule (dxv_mesh_distance), written from the rule's text.

Test helper, not collected.  Brute force: every triangle for every point, every intermediate float32 (checked), chunked over the
triangles.  `dtype=np.float64` is its twin for the accuracy checks.  The voxel centres and the normalised triangles are
surface_restated's (the ray rule's centre, the scene rule's normalisation).
"""
import numpy as np

from surface_restated import centres, normalised_tris

F32 = np.float32
NO_TRIANGLE = 0xFFFFFFFF
VOXELS_F32, UNITS_F32 = 0, 1


def _chk(t, *arrays):
    for a in arrays:
        assert a.dtype == t, a.dtype


def _dot(u, v):
    return (u[0] * v[0] + u[1] * v[1]) + u[2] * v[2]


def _seg(p, a, b, t):
    e = [b[k] - a[k] for k in range(3)]
    w = [p[k] - a[k] for k in range(3)]
    ee = _dot(e, e)
    we = _dot(w, e)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        s = np.where(ee > 0, we / ee, t(0)).astype(t)
    s = np.minimum(np.maximum(s, t(0)), t(1))
    d = [p[k] - (a[k] + s * e[k]) for k in range(3)]
    r = _dot(d, d)
    _chk(t, ee, we, s, r, *e, *w, *d)
    return r


def _face(p, a, b, c, t):
    ab = [b[k] - a[k] for k in range(3)]
    ac = [c[k] - a[k] for k in range(3)]
    ap = [p[k] - a[k] for k in range(3)]
    d00, d01, d11, d20, d21 = _dot(ab, ab), _dot(ab, ac), _dot(ac, ac), _dot(ap, ab), _dot(ap, ac)
    den = d00 * d11 - d01 * d01
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        v = (d11 * d20 - d01 * d21) / den
        w = (d00 * d21 - d01 * d20) / den
        valid = (den > 0) & (v >= 0) & (w >= 0) & (v + w <= 1)
        d = [p[k] - ((a[k] + v * ab[k]) + w * ac[k]) for k in range(3)]
        r = _dot(d, d)
    _chk(t, den, v, w, r, *d)
    return np.where(valid, r, t(np.inf)).astype(t)


def f_all(points, tris, dtype=F32):
    """f(p; tri_k) for every point and triangle: points (V, 3), tris (K, 3, 3) -> (V, K) in dtype."""
    t = dtype
    points, tris = np.asarray(points, t), np.asarray(tris, t)
    p = [points[:, None, k] for k in range(3)]
    a, b, c = ([tris[None, :, j, k] for k in range(3)] for j in range(3))
    f = np.minimum(np.minimum(np.minimum(_seg(p, a, b, t), _seg(p, b, c, t)), _seg(p, c, a, t)), _face(p, a, b, c, t))
    _chk(t, f)
    return f


def cap_of(N, band, dtype=F32):
    """R * R of a band of `band` voxels (None: no band)"""
    if not band:
        return None
    t = dtype
    h = t(2.0) / t(N)
    R = t(band) * h
    return R * R


def nearest(points, tris, index=None, cap=None, dtype=F32, chunk=256):
    """(d2 (V,), tri (V,) uint32): the minimum of f over the triangles, capped, and the smallest index among the minimisers
    (index: the triangles' indices, default their positions); NO_TRIANGLE where the cap is strictly smaller than every f."""
    t = dtype
    points = np.asarray(points, t)
    tris = np.asarray(tris, t)
    index = np.arange(len(tris), dtype=np.int64) if index is None else np.asarray(index, np.int64)
    d2 = np.full(len(points), np.inf if cap is None else cap, t)
    tri = np.full(len(points), NO_TRIANGLE, np.int64)
    for s in range(0, len(tris), chunk):
        f = f_all(points, tris[s:s + chunk], t)
        idx = index[s:s + chunk]
        m = f.min(1)
        who = np.where(f == m[:, None], idx[None, :], NO_TRIANGLE).min(1)     # smallest index among this chunk's minimisers
        better = (m < d2) | ((m == d2) & (who < tri))
        d2 = np.where(better, m, d2)
        tri = np.where(better, who, tri)
    _chk(t, d2)
    return d2, tri.astype(np.uint32)


def grid_points(N, z0=0, nz=None, dtype=F32):
    """the centres of slices [z0, z0 + nz) of an N^3 grid, (nz * N * N, 3) in the field's element order (z, y, x)"""
    nz = N - z0 if nz is None else nz
    c = centres(N, np.arange(N), dtype)
    cz = centres(N, np.arange(z0, z0 + nz), dtype)
    z, y, x = np.meshgrid(cz, -c, c, indexing="ij")
    return np.stack([x.ravel(), y.ravel(), z.ravel()], 1)


def value(d2, solid, fmt, N):
    """the field's element from float32 d2 and the grid's bytes"""
    d2 = np.asarray(d2, F32)
    d = np.sqrt(d2)
    v = d * (F32(0.5) * F32(N)) if fmt == VOXELS_F32 else d
    s = np.where(np.asarray(solid) != 0, F32(-1), F32(1))
    r = s * v
    _chk(F32, d, v, r)
    return r


def field(tris, N, grid=None, fmt=VOXELS_F32, band=0, z0=0, nz=None, index=None, chunk=256):
    """(field float32 [nz, N, N], tri uint32 [nz, N, N]) of normalised triangles tris (T, 3, 3); grid: the bytes that give the sign
    (None: all empty)"""
    nz = N - z0 if nz is None else nz
    d2, tri = nearest(grid_points(N, z0, nz), tris, index, cap_of(N, band), F32, chunk)
    solid = np.zeros(nz * N * N, np.uint8) if grid is None else np.asarray(grid).reshape(-1)
    return value(d2, solid, fmt, N).reshape(nz, N, N), tri.reshape(nz, N, N)


def field_of_mesh(vb, ib, N, grid=None, fmt=VOXELS_F32, band=0, z0=0, nz=None, bound=None):
    return field(normalised_tris(vb, ib, bound), N, grid, fmt, band, z0, nz)


# ---- the seeded soups of the rule tests: random, small, sliver and degenerate triangles in [-1, 1]^3 ---------------------------------
def soup(kind, T, seed):
    rng = np.random.default_rng(seed)
    a = rng.uniform(-1, 1, (T, 1, 3))
    if kind == "random":
        t = rng.uniform(-1, 1, (T, 3, 3))
    elif kind == "small":
        t = a + rng.uniform(-1, 1, (T, 3, 3)) * 10.0 ** rng.uniform(-4, -1, (T, 1, 1))
    elif kind == "sliver":                                               # a long edge, the third vertex almost on it
        e = rng.uniform(-1, 1, (T, 1, 3))
        s = rng.uniform(0, 1, (T, 1, 1))
        off = rng.uniform(-1, 1, (T, 1, 3)) * 10.0 ** rng.uniform(-7, -3, (T, 1, 1))
        t = np.concatenate([a, a + e, a + s * e + off], 1)
    elif kind == "degenerate":                                           # points, zero-length edges, exactly collinear vertices
        t = rng.uniform(-1, 1, (T, 3, 3)).astype(F32)
        k = np.arange(T) % 4
        t[k == 0, 1] = t[k == 0, 0]; t[k == 0, 2] = t[k == 0, 0]
        t[k == 1, 1] = t[k == 1, 0]
        t[k == 2, 2] = t[k == 2, 1]
        d = (t[k == 3, 1] - t[k == 3, 0]).astype(F32)
        t[k == 3, 1] = t[k == 3, 0] + d
        t[k == 3, 2] = t[k == 3, 0] + F32(2) * d                         # (a + 2 d: collinear up to one rounding, often exactly)
    else:
        raise ValueError(kind)
    return np.clip(t, -1, 1).astype(F32)


SOUPS = ("random", "small", "sliver", "degenerate")
