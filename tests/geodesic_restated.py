"""The geodesic distance inside a grid (include/dxv.h: dxv_geodesic*), restated twice and independently of the product's tiles:
(a) geodesic: whole-array numpy relaxation to the fixed point, 6 or 26 shifted minima per sweep;
(b) geodesic_dijkstra: Dijkstra on the explicit graph (scipy.sparse.csgraph.dijkstra, min_only=True; the integer weights are exact in float64).
Beside them the tally, the path's descent, the limit's second form and the grids the tests share.  A plain helper: no fixtures, no hooks."""
import numpy as np

SOLID, EMPTY = 0, 1
FACES, CHAMFER = 0, 1
NONE, UNREACHED = 0xFFFFFFFF, 0xFFFFFFFE
_FAR = np.int64(1) << 40


def members(grid, of):
    solid = np.asarray(grid) != 0
    return solid if of == SOLID else ~solid


def steps(metric):
    """(dz, dy, dx, weight) of the metric's neighbours in order of increasing index: dz outermost, dx innermost"""
    out = []
    for dz in (-1, 0, 1):
        for dy in (-1, 0, 1):
            for dx in (-1, 0, 1):
                e2 = dx * dx + dy * dy + dz * dz
                if e2 and (metric == CHAMFER or e2 == 1):
                    out.append((dz, dy, dx, 1 if metric == FACES else 2 + e2))
    return out


def seed_mask(shape, seeds):
    """bool [N, N, N]: "border", an array of voxel indices (iz * N + iy) * N + ix, or N^3 values of which the non-zero ones are seeds"""
    N = shape[0]
    if isinstance(seeds, str):
        assert seeds == "border"
        m = np.zeros(shape, bool)
        if N:
            m[[0, -1], :, :] = m[:, [0, -1], :] = m[:, :, [0, -1]] = True
        return m
    s = np.asarray(seeds)
    if s.ndim == 3:
        return s != 0
    m = np.zeros(N ** 3, bool)
    m[s.astype(np.int64)] = True
    return m.reshape(shape)


def _finish(D, M):
    out = np.full(M.shape, NONE, np.uint32)
    out[M] = np.where(D[M] >= _FAR, UNREACHED, D[M]).astype(np.uint32)
    return out


def geodesic(grid, of, metric, seeds="border", limit=0, sweeps=None):
    """form (a), with the limit applied while relaxing: a candidate above it is dropped"""
    M = members(grid, of)
    N = M.shape[0]
    P = np.full((N + 2,) * 3, _FAR, np.int64)                            # (a halo of "far": voxels outside the grid do not exist)
    D = P[1:-1, 1:-1, 1:-1]
    D[seed_mask(M.shape, seeds) & M] = 0
    count = 0
    while True:
        before = D.copy()
        for dz, dy, dx, w in steps(metric):
            cand = P[1 + dz:N + 1 + dz, 1 + dy:N + 1 + dy, 1 + dx:N + 1 + dx] + w
            ok = M & (cand < D)
            if limit:
                ok &= cand <= limit
            D[ok] = cand[ok]
        count += 1
        if np.array_equal(before, D):
            break
    if sweeps is not None:
        sweeps.append(count)
    return _finish(D, M)


def geodesic_dijkstra(grid, of, metric, seeds="border", limit=0):
    """form (b); the limit by its second form"""
    from scipy.sparse import coo_matrix
    from scipy.sparse.csgraph import dijkstra
    M = members(grid, of)
    N = M.shape[0]
    node = np.full(M.shape, -1, np.int64)
    K = int(M.sum())
    node[M] = np.arange(K)
    D = np.full(M.shape, _FAR, np.int64)
    S = seed_mask(M.shape, seeds) & M
    if K and S.any():
        rows, cols, vals = [], [], []
        for dz, dy, dx, w in steps(metric):
            if (dz, dy, dx) < (0, 0, 0):
                continue                                                 # (each undirected edge once)
            a = node[:N - dz, max(0, -dy):N - max(0, dy), max(0, -dx):N - max(0, dx)]
            b = node[dz:, max(0, dy):N + min(0, dy), max(0, dx):N + min(0, dx)]
            both = (a >= 0) & (b >= 0)
            rows.append(a[both]); cols.append(b[both]); vals.append(np.full(int(both.sum()), float(w)))
        g = coo_matrix((np.concatenate(vals), (np.concatenate(rows), np.concatenate(cols))), shape=(K, K)).tocsr()
        d = dijkstra(g, directed=False, indices=node[S], min_only=True)
        D[M] = np.where(np.isinf(d), _FAR, d).astype(np.int64)
    return limited(_finish(D, M), limit)


def limited(out0, limit):
    """the limit's second form: the unlimited map with every value above the limit read as UNREACHED (members only: NONE stays)"""
    if not limit:
        return out0
    return np.where((out0 < UNREACHED) & (out0 > limit), np.uint32(UNREACHED), out0).astype(np.uint32)


def tally(out):
    """{seeds_used, reached, unreached, farthest, farthest_voxel} of a map"""
    flat = np.asarray(out).reshape(-1)
    reached = flat < UNREACHED
    t = {"seeds_used": int(np.count_nonzero(flat == 0)), "reached": int(reached.sum()), "unreached": int(np.count_nonzero(flat == UNREACHED)), "farthest": 0,
         "farthest_voxel": 0xFFFFFFFF}
    if t["reached"]:
        t["farthest"] = int(flat[reached].max())
        t["farthest_voxel"] = int(np.flatnonzero(flat == t["farthest"])[0])
    return t


def path(out, metric, target):
    """the voxel indices from target down to a seed: at every voxel the FIRST neighbour q, in order of increasing index, with out(q) + w == out(p)"""
    N = out.shape[0]
    flat = out.reshape(-1)
    assert 0 <= target < N ** 3 and flat[target] < UNREACHED
    p, found = int(target), [int(target)]
    while flat[p]:
        z, y, x = p // (N * N), p // N % N, p % N
        for dz, dy, dx, w in steps(metric):
            qz, qy, qx = z + dz, y + dy, x + dx
            if 0 <= qz < N and 0 <= qy < N and 0 <= qx < N:
                q = (qz * N + qy) * N + qx
                if flat[q] < UNREACHED and int(flat[q]) + w == int(flat[p]):
                    break
        else:
            raise AssertionError(f"no neighbour of voxel {p} continues the path")
        p = q
        found.append(p)
    return np.array(found, np.uint32)


def check_path(out, metric, found, target):
    """the properties of a path: it starts at target, consecutive voxels are allowed steps, values fall by exactly the step's weight, it ends on a seed"""
    N = out.shape[0]
    flat = out.reshape(-1)
    found = [int(p) for p in found]
    assert found[0] == int(target) and flat[found[-1]] == 0 and all(flat[p] != 0 for p in found[:-1])
    weight = {(dz, dy, dx): w for dz, dy, dx, w in steps(metric)}
    for p, q in zip(found, found[1:]):
        d = (q // (N * N) - p // (N * N), q // N % N - p // N % N, q % N - p % N)
        assert d in weight and flat[q] < UNREACHED and int(flat[p]) - int(flat[q]) == weight[d], (p, q, d)


def smallest_member(grid, of):
    """[the smallest member index] as a seed list, or an empty one"""
    m = np.flatnonzero(members(grid, of).reshape(-1))
    return m[:1].astype(np.uint32)


# ---- grids ------------------------------------------------------------------------------------------------------------------------------------
def corridor(N, length):
    """a straight corridor of `length` solid voxels along x from (1, 1, 1)"""
    g = np.zeros((N, N, N), np.uint8)
    g[1, 1, 1:1 + length] = 1
    return g


def checkerboard(N):
    z, y, x = np.indices((N, N, N))
    return ((x + y + z) % 2 == 0).astype(np.uint8)


def serpentine(N, thick=2, gap=2):
    """solid slabs across z, `thick` voxels each with `gap` empty ones between, joined at alternating ends of x by a bridge: one path that crosses
    every slab from end to end"""
    g = np.zeros((N, N, N), np.uint8)
    k, z = 0, 0
    while z + thick <= N:
        g[z:z + thick, :, :] = 1
        if z + thick + gap + thick <= N:
            xs = slice(N - 2, N) if k % 2 == 0 else slice(0, 2)
            g[z + thick:z + thick + gap, :, xs] = 1
        z += thick + gap
        k += 1
    return g


def sealed_cavity(N):
    """empty space, a closed solid shell round an empty cavity"""
    g = np.zeros((N, N, N), np.uint8)
    lo, hi = N // 4, N - N // 4 - 1
    g[lo:hi + 1, lo:hi + 1, lo:hi + 1] = 1
    g[lo + 1:hi, lo + 1:hi, lo + 1:hi] = 0
    return g
