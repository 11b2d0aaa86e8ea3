"""The access radius A and the intrusion map I of include/dxv.h (dxv_access) restated in numpy, each twice and by different means:
  A  (a) a widest-path search from the seeds with a max-heap (heapq): a voxel is final when it is popped
     (b) the threshold form: {A >= t} is the union of the components of {R >= t} that hold a seed with R >= t (scipy.ndimage.label)
  I  (c) the definition: the union of the open balls of radius^2 A(c) round every c, the greatest value winning
     (d) the erode / keep-connected / dilate loop with morph_restated's closed ball, once per radius
and the grids the device tests use.  Plain helpers: no fixtures, no hooks."""
import heapq

import numpy as np
from scipy import ndimage

import geodesic_restated as gr
import morph_restated as mr
import thickness_restated as tr

SOLID, EMPTY = 0, 1
BORDER = "border"

members = tr.members
radius = tr.radius
seed_mask = gr.seed_mask
histogram = tr.histogram


def offsets(connectivity):
    assert connectivity in (6, 26)
    return [(dz, dy, dx) for dz in (-1, 0, 1) for dy in (-1, 0, 1) for dx in (-1, 0, 1)
            if (dz or dy or dx) and (connectivity == 26 or dz * dz + dy * dy + dx * dx == 1)]


def access(grid, of, connectivity, cap_sq, seeds=BORDER):
    """uint32 [N, N, N], form (a)"""
    R = radius(grid, of, cap_sq)
    N = R.shape[0]
    S = seed_mask(R.shape, seeds) & (R > 0)
    A = np.zeros(R.shape, np.int64)
    heap = [(-int(R[p]), p) for p in zip(*np.nonzero(S))]
    for _, p in heap:
        A[p] = R[p]
    heapq.heapify(heap)
    steps = offsets(connectivity)
    done = np.zeros(R.shape, bool)
    while heap:
        a, p = heapq.heappop(heap)
        if done[p]:
            continue
        done[p] = True
        for dz, dy, dx in steps:
            q = (p[0] + dz, p[1] + dy, p[2] + dx)
            if min(q) < 0 or max(q) >= N or done[q]:
                continue
            through = min(-a, int(R[q]))
            if through > A[q]:
                A[q] = through
                heapq.heappush(heap, (-through, q))
    return A.astype(np.uint32)


def access_by_thresholds(grid, of, connectivity, cap_sq, seeds=BORDER):
    """uint32 [N, N, N], form (b)"""
    R = radius(grid, of, cap_sq)
    S = seed_mask(R.shape, seeds)
    structure = ndimage.generate_binary_structure(3, 1 if connectivity == 6 else 3)
    A = np.zeros(R.shape, np.int64)
    for t in np.unique(R):
        if not t:
            continue
        labels, _ = ndimage.label(R >= t, structure)
        seeded = np.unique(labels[S & (R >= t)])
        A[np.isin(labels, seeded[seeded > 0])] = t                      # (t rising: the last threshold a voxel survives is its A)
    return A.astype(np.uint32)


def intrusion(grid, of, A):
    """uint32 [N, N, N], form (c), from an access map"""
    A = np.asarray(A).astype(np.int64)
    W = np.zeros(A.shape, np.int64)
    for v in np.unique(A):
        if v:
            W = np.maximum(W, int(v) * mr.reach(A == v, int(v) - 1))
    return np.where(members(grid, of), W, 0).astype(np.uint32)


def intrusion_by_loop(grid, of, connectivity, cap_sq, seeds=BORDER):
    """uint32 [N, N, N], form (d): from the grid alone, no access map in between"""
    m = members(grid, of)
    S = seed_mask(m.shape, seeds)
    structure = ndimage.generate_binary_structure(3, 1 if connectivity == 6 else 3)
    out = np.zeros(m.shape, np.int64)
    for r2 in range(cap_sq):
        core = m if r2 == 0 else mr.erode(m, r2)                        # {R >= r2 + 1}
        if not core.any():
            break
        labels, _ = ndimage.label(core, structure)
        seeded = np.unique(labels[S & core])
        kept = np.isin(labels, seeded[seeded > 0])                      # {A >= r2 + 1}
        out[kept if r2 == 0 else mr.dilate(kept, r2)] = r2 + 1
    return out.astype(np.uint32)


def tally(grid, of, A, seeds=BORDER):
    """{seeds_used, reached, unreached, widest, widest_voxel}"""
    m = members(grid, of)
    A = np.asarray(A)
    flat = A.reshape(-1)
    reached = int((A > 0).sum())
    return {"seeds_used": int((seed_mask(m.shape, seeds) & m).sum()), "reached": reached, "unreached": int(m.sum()) - reached, "widest": int(flat.max()) if reached else 0,
            "widest_voxel": int(np.flatnonzero(flat == flat.max())[0]) if reached else 0xFFFFFFFF}


# ---- the grids ------------------------------------------------------------------------------------------------------------------------------
def ink_bottle(N=16, width=1, sx=0, sz=0):
    """solid but for a 7^3 chamber and a channel `width` voxels wide from the face x = 0 to it, both shifted by (sx, sz): the members are the EMPTY
    voxels.  -> (grid, a voxel of the channel's axis, the chamber's centre), both (z, y, x)"""
    g = np.ones((N, N, N), np.uint8)
    h = width // 2
    g[5 + sz:12 + sz, 5:12, 6 + sx:13 + sx] = 0
    g[8 + sz - h:8 + sz + h + 1, 8 - h:8 + h + 1, 0:6 + sx] = 0
    return g, (8 + sz, 8, 3), (8 + sz, 8, 9 + sx)


def raised_twice():
    """24^3, solid but for: a 3-wide corridor from the seed along x, along y and back along x -- six tile faces -- into a 5^3 chamber, and a 1-wide
    shortcut from the seed straight to the chamber.  The chamber is reached through the shortcut first and raised through the corridor later.
    -> (grid, the seed's index, the chamber's centre (z, y, x))"""
    N = 24
    g = np.ones((N, N, N), np.uint8)
    g[2:5, 2:5, 2:22] = 0
    g[2:5, 2:21, 19:22] = 0
    g[2:5, 18:21, 7:22] = 0
    g[1:6, 17:22, 3:8] = 0
    g[3, 5:17, 3] = 0
    return g, (3 * N + 3) * N + 3, (3, 19, 5)


def staircase():
    """12^3, solid but for the voxels (k, k, k), k = 0 .. 8, and a 3^3 room behind the last: connected at 26 only; (0, 0, 0) lies on the border"""
    g = np.ones((12, 12, 12), np.uint8)
    for k in range(9):
        g[k, k, k] = 0
    g[8:11, 8:11, 8:11] = 0
    return g


def checkerboard(N):
    z, y, x = np.indices((N, N, N))
    return ((x + y + z) % 2).astype(np.uint8)


def builders():
    """(name, grid, a list of seed indices for it) of the small grids every form is run on"""
    import grid_sides
    a, _, _ = ink_bottle(16, 1)
    b, _, _ = ink_bottle(16, 3)
    c, seed, _ = raised_twice()
    out = [("bottle 1", a, [8 * 256 + 8 * 16]), ("bottle 3", b, [8 * 256 + 8 * 16, 8 * 256 + 8 * 16]), ("raised twice", c, [seed]), ("staircase", staircase(), [0, 5]),
           ("checkerboard", checkerboard(10), [1, 2, 3, 999])]
    for name, g in grid_sides.grids(18, ("random 0.3", "hollow box")):
        out.append((name, g, [0, 17, 18 ** 3 // 2 + 9, 18 ** 3 - 1]))
    return out
