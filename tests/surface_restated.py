"""An independent numpy restatement of the surface rule (DXV_MODE_SURFACE), written from the rule's text.

Test helper, not collected.  `surface_grid(tris, N)` gives the uint8 [z, y, x] grid of the closed voxel boxes that overlap at
least one closed triangle, decided by the float32 separating-axis test exactly as DESIGN §2 orders it (every intermediate is checked
to be float32); `dtype=np.float64` is its twin for cross-checks.  The candidates are only a superset: each triangle's box in voxel
units widened by one voxel; a triangle with a large box is walked column by column over its dominant axis plane, each column over
the depths its plane reaches (widened by one voxel), so that 1024^3 grids with huge triangles stay cheap.  The walk follows the EXACT
plane; the float32 test of a triangle with a vertex far outside the grid does not (its products are rounded at the far vertex's
magnitude), so such a triangle (FAR_LIMIT) tests its whole box instead.

`box_grid(tris, N)` is the truth for the candidate enumerations: the same test on every voxel of `kernel_box` (csrc/dxv_surface.h:
surface_box restated), with no column walk and no plane reasoning.
"""
import numpy as np

F32 = np.float32
FAR_LIMIT = 2.0 ** 17      # a triangle with |coordinate| * N above this tests its whole box (csrc/dxv_surface.h: kSurfaceFar, derived there)


def bound_of(vb):
    """The scene rule of DESIGN §2: c = (max + min) / 2 per axis, w = largest extent / 2, both float32."""
    p = np.ascontiguousarray(vb, F32).reshape(-1, 6)[:, :3]
    mn, mx = p.min(0), p.max(0)
    c = (mx + mn) / F32(2)
    ext = mx - mn
    w = max(ext[0], max(ext[1], ext[2])) / F32(2)
    assert c.dtype == F32 and w.dtype == F32
    return c, w


def normalised_tris(vb, ib, bound=None):
    """(T, 3 vertices, 3) float32 positions v' = (v - c) / w; bound: (c, w) of another mesh (a refit keeps its build's bound)."""
    c, w = bound_of(vb) if bound is None else bound
    p = np.ascontiguousarray(vb, F32).reshape(-1, 6)[:, :3]
    q = (p - c) / w
    assert q.dtype == F32
    return q[np.asarray(ib, np.int64).reshape(-1, 3)]


def centres(N, i, dtype=F32):
    """The ray rule's voxel centre coordinate (i + .5) / N * 2 - 1 in dtype (y is the negation of this)."""
    t = dtype
    v = (np.asarray(i).astype(t) + t(0.5)) / t(N) * t(2) - t(1)
    assert v.dtype == t
    return v


def _chk(dtype, *arrays):
    for a in arrays:
        assert a.dtype == dtype, a.dtype


def overlap(a, b, d, c, h, dtype=F32):
    """The test: a, b, d (K, 3) triangle vertices, c (K, 3) box centres, h the half size; bool (K,)."""
    t = dtype
    a, b, d, c = (np.asarray(x, t) for x in (a, b, d, c))
    h = t(h)
    v0, v1, v2 = a - c, b - c, d - c
    _chk(t, v0, v1, v2)
    ok = np.ones(len(a), bool)
    for k in range(3):
        lo = np.minimum(np.minimum(v0[:, k], v1[:, k]), v2[:, k])
        hi = np.maximum(np.maximum(v0[:, k], v1[:, k]), v2[:, k])
        ok &= ~((lo > h) | (hi < -h))
    e0, e1, e2 = v1 - v0, v2 - v1, v0 - v2
    _chk(t, e0, e1, e2)
    for e in (e0, e1, e2):
        for i in range(3):
            j, k = (i + 1) % 3, (i + 2) % 3
            p = [e[:, j] * v[:, k] - e[:, k] * v[:, j] for v in (v0, v1, v2)]
            r = np.abs(e[:, j]) * h + np.abs(e[:, k]) * h
            _chk(t, r, *p)
            ok &= ~((np.minimum(np.minimum(p[0], p[1]), p[2]) > r) | (np.maximum(np.maximum(p[0], p[1]), p[2]) < -r))
    nx = e0[:, 1] * e1[:, 2] - e0[:, 2] * e1[:, 1]
    ny = e0[:, 2] * e1[:, 0] - e0[:, 0] * e1[:, 2]
    nz = e0[:, 0] * e1[:, 1] - e0[:, 1] * e1[:, 0]
    n = (nx, ny, nz)
    vmin = [np.where(n[k] > 0, -h, h).astype(t) - v0[:, k] for k in range(3)]
    vmax = [np.where(n[k] > 0, h, -h).astype(t) - v0[:, k] for k in range(3)]
    smin = (nx * vmin[0] + ny * vmin[1]) + nz * vmin[2]
    smax = (nx * vmax[0] + ny * vmax[1]) + nz * vmax[2]
    _chk(t, nx, ny, nz, smin, smax, *vmin, *vmax)
    ok &= ~(smin > 0)
    ok &= smax >= 0
    return ok


def _vox(p, N):
    """Voxel-unit coordinates (float64) of normalised positions (..., 3): voxel i spans [i, i + 1]; y is flipped."""
    p = np.asarray(p, np.float64)
    q = np.empty_like(p)
    q[..., 0] = (p[..., 0] + 1.0) * N / 2
    q[..., 1] = (1.0 - p[..., 1]) * N / 2
    q[..., 2] = (p[..., 2] + 1.0) * N / 2
    return q


def _boxes(tris, N):
    q = _vox(tris, N)
    lo = np.clip(np.floor(q.min(1)) - 1, 0, N - 1).astype(np.int64)
    hi = np.clip(np.floor(q.max(1)) + 1, 0, N - 1).astype(np.int64)
    empty = (np.floor(q.max(1)) + 1 < 0).any(1) | (np.floor(q.min(1)) - 1 > N - 1).any(1)
    return lo, hi, empty


def _test_and_set(grid, tris, tid, ix, iy, iz, N, dtype):
    if not len(tid):
        return
    t = dtype
    c = np.stack([centres(N, ix, t), -centres(N, iy, t), centres(N, iz, t)], 1)
    tr = tris[tid].astype(t)
    ok = overlap(tr[:, 0], tr[:, 1], tr[:, 2], c, t(1) / t(N), t)
    grid[iz[ok], iy[ok], ix[ok]] = 1


def _columns(tri, lo, hi, N):
    """Candidate voxels (ix, iy, iz) of one large triangle: columns along the normal's dominant axis, each over the depths its
    plane reaches above the column's square, widened by one voxel and clipped to the box."""
    q = _vox(tri, N)
    e1, e2 = q[1] - q[0], q[2] - q[0]
    n = np.cross(e1, e2)
    w = int(np.argmax(np.abs(n)))
    u, v = (w + 1) % 3, (w + 2) % 3
    cu, cv = np.meshgrid(np.arange(lo[u], hi[u] + 1), np.arange(lo[v], hi[v] + 1), indexing="ij")
    cu, cv = cu.ravel(), cv.ravel()
    if abs(n[w]) > 1e-9 * np.abs(e1).max() * np.abs(e2).max():
        depth = [q[0, w] - (n[u] * (cu + du - q[0, u]) + n[v] * (cv + dv - q[0, v])) / n[w] for du in (0, 1) for dv in (0, 1)]
        k0 = np.clip(np.floor(np.min(depth, 0)) - 1, lo[w], hi[w] + 1).astype(np.int64)
        k1 = np.clip(np.floor(np.max(depth, 0)) + 1, lo[w] - 1, hi[w]).astype(np.int64)
    else:
        k0 = np.full(cu.shape, lo[w], np.int64)
        k1 = np.full(cu.shape, hi[w], np.int64)
    cnt = np.maximum(k1 - k0 + 1, 0)
    rep = np.repeat(np.arange(len(cu)), cnt)
    k = k0[rep] + (np.arange(len(rep)) - np.repeat(np.cumsum(cnt) - cnt, cnt))
    at = [None] * 3
    at[u], at[v], at[w] = cu[rep], cv[rep], k
    return at[0], at[1], at[2]


def surface_grid(tris, N, dtype=F32, chunk=1 << 22, large=4096):
    """uint8 [N, N, N] (z, y, x) grid of the surface rule for normalised triangles tris (T, 3, 3)."""
    tris = np.ascontiguousarray(tris, F32)
    grid = np.zeros((N, N, N), np.uint8)
    lo, hi, empty = _boxes(tris, N)
    ext = np.where(empty[:, None], 0, hi - lo + 1)
    cnt = ext.prod(1)
    far = np.abs(tris.astype(np.float64)).max((1, 2)) * N > FAR_LIMIT
    small = np.nonzero((cnt > 0) & ((cnt <= large) | far))[0]
    # small boxes: every voxel of the box, a batch of triangles at a time
    ends = np.cumsum(cnt[small])
    start = 0
    while start < len(small):
        stop = int(np.searchsorted(ends, (ends[start - 1] if start else 0) + chunk, "right"))
        stop = max(stop, start + 1)
        sel = small[start:stop]
        c = cnt[sel]
        tid = np.repeat(sel, c)
        off = np.arange(len(tid)) - np.repeat(np.cumsum(c) - c, c)
        ex, ey = ext[tid, 0], ext[tid, 1]
        ix = lo[tid, 0] + off % ex
        iy = lo[tid, 1] + (off // ex) % ey
        iz = lo[tid, 2] + off // (ex * ey)
        _test_and_set(grid, tris, tid, ix, iy, iz, N, dtype)
        start = stop
    for t in np.nonzero((cnt > large) & ~far)[0]:
        ix, iy, iz = _columns(tris[t], lo[t], hi[t], N)
        for s in range(0, len(ix), chunk):
            sl = slice(s, s + chunk)
            _test_and_set(grid, tris, np.full(len(ix[sl]), t), ix[sl], iy[sl], iz[sl], N, dtype)
    return grid


def brute_grid(tris, N, dtype=F32):
    """The rule applied to every voxel of the grid against every triangle (small N only)."""
    tris = np.ascontiguousarray(tris, F32)
    grid = np.zeros((N, N, N), np.uint8)
    iz, iy, ix = (a.ravel() for a in np.meshgrid(np.arange(N), np.arange(N), np.arange(N), indexing="ij"))
    for t in range(len(tris)):
        _test_and_set(grid, tris, np.full(len(ix), t), ix, iy, iz, N, dtype)
    return grid


def kernel_box(tri, N):
    """surface_box (csrc/dxv_surface.h) restated in float32: lo, hi per axis (x, y, z), or None when it is empty."""
    tri = np.asarray(tri, F32)
    if not np.isfinite(tri).all() or np.abs(tri).max() >= F32(1e30):
        return None
    half, m = F32(0.5) * F32(N), F32(0.0625)
    lo, hi = [], []
    for k in range(3):
        mn, mx = tri[:, k].min(), tri[:, k].max()
        u0 = (F32(1) - mx) * half if k == 1 else (mn + F32(1)) * half
        u1 = (F32(1) - mn) * half if k == 1 else (mx + F32(1)) * half
        u0 = min(max(np.floor(u0 - m), F32(-1)), F32(N))
        u1 = min(max(np.floor(u1 + m), F32(-1)), F32(N))
        lo.append(0 if u0 < 0 else int(u0))
        hi.append(N - 1 if u1 > N - 1 else int(u1))
        if lo[k] > hi[k]:
            return None
    return lo, hi


def box_grid(tris, N, counts=None):
    """uint8 [N, N, N] (z, y, x): the float32 test applied to EVERY voxel of every triangle's kernel_box -- no walk, no plane.
    counts: a list that receives (voxels in the box, voxels accepted) per triangle."""
    tris = np.ascontiguousarray(tris, F32).reshape(-1, 3, 3)
    grid = np.zeros((N, N, N), np.uint8)
    for t, tri in enumerate(tris):
        box = kernel_box(tri, N)
        if box is None:
            if counts is not None:
                counts.append((0, 0))
            continue
        lo, hi = box
        iz, iy, ix = (a.ravel() for a in np.meshgrid(*(np.arange(lo[k], hi[k] + 1) for k in (2, 1, 0)), indexing="ij"))
        one = np.zeros_like(grid)
        _test_and_set(one, tris, np.full(len(ix), t), ix, iy, iz, N, F32)
        grid |= one
        if counts is not None:
            counts.append((len(ix), int(one.sum())))
    return grid


def surface_of_mesh(vb, ib, N, bound=None, dtype=F32):
    return surface_grid(normalised_tris(vb, ib, bound), N, dtype)
