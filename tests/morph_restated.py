"""Morphology by the Euclidean ball restated in numpy, twice, from the rule's text alone (include/dxv.h over dxv_morph_async):

    solid(p) iff byte(p) != 0;   B = { v in Z^3 : vx^2 + vy^2 + vz^2 <= r2 }
    DILATE(p) = 1 iff there is q in the grid with solid(q)  and |p - q|^2 <= r2
    ERODE(p)  = 1 iff solid(p) and there is NO q in the grid with !solid(q) and |p - q|^2 <= r2
    OPEN = DILATE(ERODE(grid)),  CLOSE = ERODE(DILATE(grid));  voxels outside the grid do not exist

1. `morph`: the OR of the grid shifted by every offset of B.  For DILATE the grid is padded with zeros; for ERODE the COMPLEMENT is shifted and
   is padded with "not empty" -- zeros again --, and the result is the solid voxels the shifted complement does not reach.
2. `morph_by_distance`: the threshold of tests/distance_restated.py's squared distance field, d = DXV_DIST_SQ_I32 of the same grid:
   DILATE(p) == solid(p) || d(p) <= r2, ERODE(p) == solid(p) && -d(p) > r2.  This one serves large r2, where B has 10^5 offsets and more.

No masks, no planes, no separable passes: nothing here shares a line of thought with the product's kernels beyond the rule."""
import hashlib

import numpy as np

import distance_restated as dr

DILATE, ERODE, OPEN, CLOSE = 0, 1, 2, 3
OPS = (DILATE, ERODE, OPEN, CLOSE)
MAX_RADIUS_SQ = 4096


def ball_offsets(r2):
    """every (dz, dy, dx) of B"""
    R = int(np.floor(np.sqrt(r2)))
    while (R + 1) ** 2 <= r2:
        R += 1
    while R * R > r2:
        R -= 1
    a = np.arange(-R, R + 1)
    dz, dy, dx = np.meshgrid(a, a, a, indexing="ij")
    keep = dz * dz + dy * dy + dx * dx <= r2
    return list(zip(dz[keep].tolist(), dy[keep].tolist(), dx[keep].tolist()))


def _span(d, n):
    """the slices (of the target, of the source) of a shift by d along an axis of n: target[i] takes source[i + d]"""
    lo, hi = max(0, -d), min(n, n - d)
    return (slice(lo, hi), slice(lo + d, hi + d)) if lo < hi else None


def reach(member, r2):
    """bool [N, N, N]: the voxels of the grid within the ball of a voxel where `member` is true; what lies outside the grid is no member"""
    member = np.asarray(member, bool)
    out = np.zeros_like(member)
    for dz, dy, dx in ball_offsets(r2):
        spans = [_span(d, n) for d, n in zip((dz, dy, dx), member.shape)]
        if any(s is None for s in spans):
            continue
        out[tuple(s[0] for s in spans)] |= member[tuple(s[1] for s in spans)]
    return out


def dilate(solid, r2):
    return reach(solid, r2)


def erode(solid, r2):
    solid = np.asarray(solid, bool)
    return solid & ~reach(~solid, r2)


def _compose(op, d, e, grid, r2):
    solid = np.asarray(grid) != 0
    if op == DILATE:
        out = d(solid, r2)
    elif op == ERODE:
        out = e(solid, r2)
    elif op == OPEN:
        out = d(e(solid, r2), r2)
    elif op == CLOSE:
        out = e(d(solid, r2), r2)
    else:
        raise ValueError(f"unknown operation {op!r}")
    return out.astype(np.uint8)


def morph(grid, op, r2):
    """uint8 [N, N, N] of 0 / 1: the morphed grid, by shifts"""
    return _compose(op, dilate, erode, grid, r2)


def _dilate_by_distance(solid, r2):
    return solid | (dr.distance_sq(solid.astype(np.uint8)) <= r2)


def _erode_by_distance(solid, r2):
    return solid & (-dr.distance_sq(solid.astype(np.uint8)).astype(np.int64) > r2)


def morph_by_distance(grid, op, r2):
    """uint8 [N, N, N] of 0 / 1: the morphed grid, by thresholds of the restated distance field"""
    return _compose(op, _dilate_by_distance, _erode_by_distance, grid, r2)


def counts(before, after):
    """(voxels set, voxels cleared): what dxv_morph_info reports"""
    was, now = np.asarray(before) != 0, np.asarray(after) != 0
    return int(np.count_nonzero(now & ~was)), int(np.count_nonzero(was & ~now))


def packed_sha(grid):
    """SHA-256 of the grid packed to a bit per voxel (voxel 8j + k in bit k of byte j, linear order): what tests/golden/morph.json holds"""
    return hashlib.sha256(np.packbits(np.asarray(grid).reshape(-1) != 0, bitorder="little").tobytes()).hexdigest()


# ---- the sealing example (the issue's numbers; tests/test_morph_rule.py pins them) ----------------------------------------------------------
def holed_shell(N=32, hole=2.3):
    """(the 2-voxel sphere shell 100 <= |p - c|^2 <= 144 at c = 15.5 with the hole z > c, (x-c)^2 + (y-c)^2 <= hole^2 cut out, the whole shell)"""
    c = (N - 1) / 2.0
    z, y, x = np.indices((N, N, N))
    d2 = (x - c) ** 2 + (y - c) ** 2 + (z - c) ** 2
    shell = (d2 >= 100) & (d2 <= 144)
    cut = shell & (z > c) & ((x - c) ** 2 + (y - c) ** 2 <= hole * hole)
    return (shell & ~cut).astype(np.uint8), shell.astype(np.uint8)
