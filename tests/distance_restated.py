"""An independent numpy restatement of the signed distance field of a grid (include/dxv.h: dxv_distance), written from
the rule's text:

    d2(p) = min over voxels q of the same grid with solid(q) != solid(p) of |p - q|^2      (integers, voxel units, centre to centre)
    DXV_DIST_SQ_I32:  s(p) * d2(p),  s = -1 for a solid voxel (byte != 0), +1 for an empty one;  no such q: s(p) * 0x7fffffff
    DXV_DIST_F32:     s(p) * sqrtf((float)d2(p));  no such q: s(p) * inf

Brute force and separable: along each axis in turn the minimum over j of (i - j)^2 + f(j), every j tried against the table of
(i - j)^2, in int64; once for the distance to the nearest solid voxel, once for the nearest empty one.  No stack, no envelope, no
scipy: nothing here shares a line of thought with the product's scans beyond the rule."""
import numpy as np

NONE = 0x7fffffff
_BIG = 1 << 40


def _min_plus(f, axis):
    """g[.., i, ..] = min over j of (i - j)^2 + f[.., j, ..] along `axis`"""
    n = f.shape[axis]
    i = np.arange(n, dtype=np.int64)
    table = (i[:, None] - i[None, :]) ** 2                          # [i, j]
    rows = np.moveaxis(f, axis, -1).reshape(-1, n)
    out = np.empty_like(rows)
    step = max(1, (1 << 25) // (n * n))                              # rows per piece: about 256 MB of int64 sums at a time
    for r in range(0, len(rows), step):
        out[r:r + step] = (rows[r:r + step, None, :] + table[None]).min(axis=-1)
    shape = list(f.shape)
    shape.append(shape.pop(axis))
    return np.moveaxis(out.reshape(shape), -1, axis)


def nearest_sq(feature):
    """int64 [z, y, x]: squared distance from every voxel to the nearest voxel where `feature` is true (>= 2^40 where there is none)"""
    f = np.where(feature, 0, _BIG).astype(np.int64)
    for axis in (2, 1, 0):
        f = _min_plus(f, axis)
    return f


def distance_sq(grid):
    """DXV_DIST_SQ_I32 of a uint8 [z, y, x] grid"""
    solid = np.asarray(grid) != 0
    d2 = np.where(solid, nearest_sq(~solid), nearest_sq(solid))
    d2 = np.where(d2 >= _BIG, NONE, d2)
    return np.where(solid, -d2, d2).astype(np.int32)


def distance_f32(grid):
    """DXV_DIST_F32 of a uint8 [z, y, x] grid"""
    return to_f32(distance_sq(grid))


def to_f32(sq):
    """the float form of an int32 field: s * sqrt((float)d2) in float32 (numpy's float32 sqrt is correctly rounded), s * inf at the sentinel"""
    sq = np.asarray(sq)
    mag = np.abs(sq.astype(np.int64))
    root = np.sqrt(mag.astype(np.float32))
    root = np.where(mag == NONE, np.float32(np.inf), root).astype(np.float32)
    return np.where(sq < 0, -root, root).astype(np.float32)
