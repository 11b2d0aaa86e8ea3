"""The line-of-sight rule of include/dxv.h restated in numpy, twice, with its tally and its edit; and the builders of the grids its tests use.
  (a) walk      the literal rule: for every member and every direction, walk back along the line until the grid ends; sides up to 8
  (b) sight     the plane recurrence V_d(c) = M(c) and (c - d outside the grid or V_d(c - d)), with shifted arrays, plane by plane along an
                axis on which d moves
Grids are uint8 [N, N, N] indexed (z, y, x); a map is uint32 of the same shape.  Bit b(d) = (dz + 1) * 9 + (dy + 1) * 3 + (dx + 1)."""
import numpy as np

SOLID, EMPTY = 0, 1
ALL = 0x07FFDFFF
BITS = [b for b in range(27) if b != 13]


def bit(dx, dy, dz):
    return (dz + 1) * 9 + (dy + 1) * 3 + (dx + 1)


def direction(b):
    return b % 3 - 1, b // 3 % 3 - 1, b // 9 - 1


def axis_bits(a):
    """the two bits of axis a as a mask"""
    return (1 << (14 + a)) | (1 << (12 - a))


def members(grid, of):
    g = np.asarray(grid)
    return (g != 0) if of == SOLID else (g == 0)


def walk(grid, of, directions):
    """(a): the literal line walk"""
    M = members(grid, of)
    N = M.shape[0]
    assert N <= 8
    out = np.zeros(M.shape, np.uint32)
    for z, y, x in zip(*np.nonzero(M)):
        for b in BITS:
            if not directions >> b & 1:
                continue
            dx, dy, dz = direction(b)
            cz, cy, cx = z - dz, y - dy, x - dx
            seen = True
            while 0 <= cz < N and 0 <= cy < N and 0 <= cx < N:
                if not M[cz, cy, cx]:
                    seen = False
                    break
                cz, cy, cx = cz - dz, cy - dy, cx - dx
            if seen:
                out[z, y, x] |= np.uint32(1 << b)
    return out


def shifted(P, dy, dx):
    """P moved by (dy, dx) in a plane: out[y, x] = P[y - dy, x - dx], True where that is outside"""
    N = P.shape[0]
    out = np.ones_like(P)
    ys, yd = (slice(0, N - 1), slice(1, N)) if dy > 0 else (slice(1, N), slice(0, N - 1)) if dy < 0 else (slice(None), slice(None))
    xs, xd = (slice(0, N - 1), slice(1, N)) if dx > 0 else (slice(1, N), slice(0, N - 1)) if dx < 0 else (slice(None), slice(None))
    out[yd, xd] = P[ys, xs]
    return out


def plane_of(grid, of, b):
    """V_d as a bool array, by the recurrence"""
    M = members(grid, of)
    N = M.shape[0]
    dx, dy, dz = direction(b)
    # bring an axis on which d moves to the front, in the order the recurrence needs: plane k depends on plane k - 1
    if dz:
        A, step, inplane = M, dz, (dy, dx)
    elif dy:
        A, step, inplane = M.transpose(1, 0, 2), dy, (0, dx)
    else:
        A, step, inplane = M.transpose(2, 0, 1), dx, (0, 0)
    V = np.zeros_like(A)
    order = range(N) if step > 0 else range(N - 1, -1, -1)
    before = np.ones((N, N), bool)
    for k in order:
        V[k] = A[k] & shifted(before, *inplane)
        before = V[k]
    if dz:
        return V
    return V.transpose(1, 0, 2) if dy else V.transpose(1, 2, 0)


def sight(grid, of, directions=ALL):
    """(b): the map by the plane recurrence"""
    out = np.zeros(np.asarray(grid).shape, np.uint32)
    for b in BITS:
        if directions >> b & 1:
            out |= plane_of(grid, of, b).astype(np.uint32) << np.uint32(b)
    return out


def tally(grid, of, field, directions):
    """{members, seen [27], neither [13], count [27]} of a map made with `directions`"""
    M = members(grid, of)
    F = np.asarray(field, np.uint32)
    seen, neither, count = np.zeros(27, np.uint64), np.zeros(13, np.uint64), np.zeros(27, np.uint64)
    for b in BITS:
        if directions >> b & 1:
            seen[b] = np.count_nonzero(F >> np.uint32(b) & 1)
    for a in range(13):
        if directions & axis_bits(a) == axis_bits(a):
            neither[a] = np.count_nonzero(M & ((F & np.uint32(axis_bits(a))) == 0))
    pop = np.zeros(F.shape, np.int64)
    for b in BITS:
        pop += (F >> np.uint32(b) & 1).astype(np.int64)
    count[:] = np.bincount(pop[M], minlength=27)[:27]
    return {"members": int(M.sum()), "seen": seen, "neither": neither, "count": count}


def same_tally(a, b):
    return a["members"] == b["members"] and all(np.array_equal(np.asarray(a[k], np.uint64), np.asarray(b[k], np.uint64)) for k in ("seen", "neither", "count"))


def sight_fill(grid, of, field, directions):
    """the grid after the edit: every member whose word shares no bit with `directions` changes kind"""
    g = np.asarray(grid, np.uint8).copy()
    hidden = members(g, of) & ((np.asarray(field, np.uint32) & np.uint32(directions)) == 0)
    g[hidden] = 1 if of == EMPTY else 0
    return g


def mirrored_bits(word, axis):
    """a map's words with the bits of d and of d mirrored along `axis` ("x", "y", "z") exchanged"""
    w = np.asarray(word, np.uint32)
    out = np.zeros_like(w)
    for b in BITS:
        dx, dy, dz = direction(b)
        m = bit(-dx if axis == "x" else dx, -dy if axis == "y" else dy, -dz if axis == "z" else dz)
        out |= (w >> np.uint32(b) & np.uint32(1)) << np.uint32(m)
    return out


# ---- builders ---------------------------------------------------------------------------------------------------------------------------------
def plate_with_pinhole(N=16, hole=(5, 9)):
    """the plate z = N / 2, solid, with one hole at (y, x) = hole"""
    g = np.zeros((N, N, N), np.uint8)
    g[N // 2] = 1
    g[N // 2, hole[0], hole[1]] = 0
    return g


def t_slot(N=16):
    """a solid block with a T-shaped slot cut through it along x: open at both x faces and at the top (z = N - 1) through a narrow neck, the
    wide part below the neck undercut for every pull but the one along x"""
    g = np.ones((N, N, N), np.uint8)
    c = N // 2
    g[N - 5:, c - 1:c + 1, :] = 0          # the neck, two voxels wide, from the top face down
    g[N - 9:N - 5, c - 4:c + 4, :] = 0     # the wide part below it
    return g
