"""The local thickness of a grid restated in numpy, three times, from the rule's text alone (include/dxv.h over dxv_thickness_async):

    M = the members: of = 0 the voxels with byte != 0, of = 1 the voxels with byte == 0; only voxels inside the grid exist
    D2(c) = min over voxels q of the grid, q not in M, of |c - q|^2          for c in M (no such q: +infinity)
    R(c)  = min(D2(c), cap_sq)
    W(p)  = max { R(c) : c in M, |p - c|^2 < R(c) }  for p in M,   W(p) = 0 for p not in M

(a) `thickness`: by values -- for each distinct v of R, W = max(W, v * reach({R == v}, v - 1)), with morph_restated.reach and distance_restated.
(b) `thickness_by_openings`: W(p) = 1 + max { r2 in 0 .. cap_sq - 1 : p in OPEN(r2) }, OPEN(0) = M, looping morph_restated.morph(OPEN, r2).
(c) `thickness_at`: per voxel -- W(p) = max over all members c of R(c) where |p - c|^2 < R(c), one vectorised pass per p.

No culls, no work items, no atomics: nothing here shares a line of thought with the product's kernels beyond the rule."""
import hashlib

import numpy as np

import distance_restated as dr
import morph_restated as mr

SOLID, EMPTY = 0, 1
MIN_CAP_SQ, MAX_CAP_SQ = 2, 4096


def members(grid, of):
    solid = np.asarray(grid) != 0
    return solid if of == SOLID else ~solid


def radius(grid, of, cap_sq):
    """int64 [N, N, N]: R on members, 0 elsewhere"""
    m = members(grid, of)
    d2 = dr.nearest_sq(~m)                                             # >= 2^40 where nothing lies outside M
    return np.where(m, np.minimum(d2, cap_sq), 0).astype(np.int64)


def thickness(grid, of, cap_sq):
    """uint32 [N, N, N], form (a)"""
    R = radius(grid, of, cap_sq)
    W = np.zeros(R.shape, np.int64)
    for v in np.unique(R):
        if v:
            W = np.maximum(W, int(v) * mr.reach(R == v, int(v) - 1))
    return W.astype(np.uint32)


def thickness_by_openings(grid, of, cap_sq):
    """uint32 [N, N, N], form (b)"""
    m = members(grid, of)
    W = m.astype(np.int64)                                             # OPEN(0) = M
    as_grid = m.astype(np.uint8)
    for r2 in range(1, cap_sq):
        W = np.where(mr.morph(as_grid, mr.OPEN, r2) != 0, r2 + 1, W)
    return W.astype(np.uint32)


def thickness_at(grid, of, cap_sq, points, R=None):
    """[len(points)] of W at the (z, y, x) of `points`, form (c); R: radius(grid, of, cap_sq) where the caller has it already"""
    R = radius(grid, of, cap_sq) if R is None else R
    z, y, x = np.indices(R.shape)
    out = []
    for pz, py, px in points:
        d2 = (z - pz) ** 2 + (y - py) ** 2 + (x - px) ** 2
        reach = R[d2 < R]
        out.append(int(reach.max()) if R[pz, py, px] and reach.size else 0)
    return np.array(out, np.uint32)


def histogram(W, cap_sq):
    """uint64 [cap_sq + 1]: bin v = the voxels with W == v"""
    return np.bincount(np.asarray(W).reshape(-1), minlength=cap_sq + 1).astype(np.uint64)


def thickness_voxels(W):
    """2 sqrt(W) - 1 on members, 0 elsewhere, float32: the diameter in voxels of the largest centred ball through the voxel"""
    W = np.asarray(W)
    return np.where(W > 0, np.float32(2) * np.sqrt(W.astype(np.float32)) - np.float32(1), np.float32(0)).astype(np.float32)


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def balls(N, seed, count=5, rmin=1.5, rmax=None):
    """uint8 [N, N, N]: a seeded union of balls"""
    rng = np.random.default_rng(seed)
    rmax = rmax or N / 4.0
    z, y, x = np.indices((N, N, N))
    g = np.zeros((N, N, N), bool)
    for _ in range(count):
        c = rng.uniform(0, N - 1, 3)
        r = rng.uniform(rmin, rmax)
        g |= (z - c[0]) ** 2 + (y - c[1]) ** 2 + (x - c[2]) ** 2 <= r * r
    return g.astype(np.uint8)


CAP_LADDER = (2, 3, 4, 5, 9, 10, 17, 26, 101)                           # the caps the rule test and the device test take on ladder_grid()


def ladder_grid():
    """the 40^3 union of balls of the cap ladder"""
    return balls(40, 3, count=8, rmax=12)
