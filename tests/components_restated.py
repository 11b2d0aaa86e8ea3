"""Connected components restated in numpy, from the rule's text alone (include/dxv.h over dxv_components_async):

    member(p)    of = SOLID: byte(p) != 0      of = EMPTY: byte(p) == 0
    adjacent     p != q, both inside the grid, |dx|,|dy|,|dz| <= 1, and for connectivity 6: |dx|+|dy|+|dz| == 1; for 26: any
    component    a class of the transitive closure of `adjacent` over the members
    first(C)     the smallest linear index (iz*N + iy)*N + ix of C's voxels
    numbering    components 1 .. K by ascending first(C)
    labels[p]    the number of p's component, 0 when !member(p)
    table[k-1]   first, voxels, lo[3] (x, y, z), hi[3], flags (bit 0: a voxel on the grid's border)

Every member starts with its own linear index; every step gives it the smallest value among itself and its adjacent members, until a
step changes nothing: then every member holds first(C).  The roots are ranked, the table is bincount and minima / maxima per label.
No scipy, no union-find, no bit tricks; the grids the tests restate are small enough for the diameter of their components in whole-grid
steps."""
import numpy as np

SOLID, EMPTY = 0, 1
LARGEST, MIN_VOXELS, BORDER = 0, 1, 2
RECORD = np.dtype([("first", "<u4"), ("voxels", "<u4"), ("lo", "<u2", (3,)), ("hi", "<u2", (3,)), ("flags", "<u4")])


def members(grid, of):
    g = np.asarray(grid)
    return g != 0 if of == SOLID else g == 0


def offsets(connectivity):
    assert connectivity in (6, 26)
    out = []
    for dz in (-1, 0, 1):
        for dy in (-1, 0, 1):
            for dx in (-1, 0, 1):
                n = abs(dx) + abs(dy) + abs(dz)
                if n and (connectivity == 26 or n == 1):
                    out.append((dz, dy, dx))
    return out


def _pair(d, n):
    """slices (to, from) along one axis of length n for offset d: to[i] takes from[i + d]"""
    if d == 0:
        return slice(0, n), slice(0, n)
    return (slice(0, n - 1), slice(1, n)) if d > 0 else (slice(1, n), slice(0, n - 1))


def firsts(grid, of=SOLID, connectivity=6):
    """uint32 [N, N, N]: first(C) of every member's component, N^3 for a voxel that is no member"""
    m = members(grid, of)
    N = m.shape[0]
    none = np.uint32(N ** 3)
    value = np.where(m, np.arange(N ** 3, dtype=np.uint32).reshape(N, N, N), none)
    pairs = [tuple(zip(*(_pair(d, N) for d in off))) for off in offsets(connectivity)]
    while True:
        new = value.copy()
        for to, frm in pairs:
            np.minimum(new[to], value[frm], out=new[to])
        new[~m] = none
        if np.array_equal(new, value):
            return value
        value = new


def label(grid, of=SOLID, connectivity=6):
    """(labels uint32 [N, N, N], table [K] of RECORD)"""
    m = members(grid, of)
    N = m.shape[0]
    value = firsts(grid, of, connectivity)
    roots = np.unique(value[m])                                         # ascending first(C)
    K = len(roots)
    labels = np.zeros((N, N, N), np.uint32)
    labels[m] = (np.searchsorted(roots, value[m]) + 1).astype(np.uint32)
    table = np.zeros(K, RECORD)
    if K:
        z, y, x = np.nonzero(m)
        k = labels[m].astype(np.int64) - 1
        table["first"] = roots
        table["voxels"] = np.bincount(k, minlength=K)
        order = np.argsort(k, kind="stable")
        starts = np.searchsorted(k[order], np.arange(K))
        for axis, c in enumerate((x, y, z)):
            table["lo"][:, axis] = np.minimum.reduceat(c[order], starts)
            table["hi"][:, axis] = np.maximum.reduceat(c[order], starts)
        border = (x == 0) | (x == N - 1) | (y == 0) | (y == N - 1) | (z == 0) | (z == N - 1)
        table["flags"] = (np.bincount(k, weights=border, minlength=K) > 0).astype(np.uint32)
    return labels, table


def keep(table, rule, arg=0):
    """bool [K]: the components a select rule keeps"""
    K = len(table)
    if rule == LARGEST:
        out = np.zeros(K, bool)
        if K:
            out[int(np.argmax(table["voxels"]))] = True                 # (argmax: the first of equal maxima, the smaller number)
        return out
    if rule == MIN_VOXELS:
        return table["voxels"] >= arg
    assert rule == BORDER
    return (table["flags"] & 1) != 0


def select(grid, labels, table, of, rule, arg=0):
    """(the edited grid, (kept, dropped, voxels_changed))"""
    kept = keep(table, rule, arg)
    drop = np.zeros(len(table) + 1, bool)
    drop[1:] = ~kept
    gone = drop[labels]
    out = np.array(grid, np.uint8, copy=True)
    out[gone] = 0 if of == SOLID else 1
    return out, (int(kept.sum()), int((~kept).sum()), int(gone.sum()))


def checkerboard(N):
    z, y, x = np.indices((N, N, N))
    return ((x + y + z) & 1).astype(np.uint8)


def one_voxel(N):
    g = np.zeros((N, N, N), np.uint8)
    g[N - 1, 0, N // 2] = 1
    return g
