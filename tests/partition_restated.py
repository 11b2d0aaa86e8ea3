"""The maximal-ball partition of a grid restated in numpy, twice, from the rule's text alone (include/dxv.h over dxv_partition_async):

    M = the members: of = 0 the voxels with byte != 0, of = 1 the voxels with byte == 0; only voxels inside the grid exist
    R(v) = min(D2(v), cap_sq) for v in M (D2: the smallest |v - q|^2 to a voxel q of the grid outside M; none: +infinity), 0 elsewhere
    u above v iff R(u) > R(v), or R(u) == R(v) and index(u) < index(v),   index(v) = (z N + y) N + x
    parent(c) = the highest voxel of { u in the grid : |u - c|^2 <= R(c) };  root(c) = where the chain of parents ends
    one region per root, numbered 1 .. K by ascending index(root); label(v) = the number of root(v) on members, 0 elsewhere
    one throat per unordered pair of labels that share a face p, q = p + e (e in +x, +y, +z; both members; labels differ):
    faces, neck_sq = max min(R(p), R(q)), neck_voxel = the smallest index(p) that attains it

(a) `partition`: vectorised.  The order as 64-bit keys R << 32 | (0xFFFFFFFF - index); the ball row by row -- for every (dz, dy) one maximum of
    the keys over the row's span of x, through a table of running maxima of every power-of-two length --, the centres sorted by R so that a row
    takes only those whose ball reaches it; pointer jumping; np.unique for the numbering and for the pairs of labels.
(b) `partition_literal`: the definition read voxel by voxel in plain Python, tuples for the order, dictionaries for the throats; N <= 12.

No mips, no pruning, no atomics: nothing here shares a line of thought with the product's kernels beyond the rule."""
import hashlib

import numpy as np

import thickness_restated as tr

SOLID, EMPTY = 0, 1
MIN_CAP_SQ, MAX_CAP_SQ = 1, 4096
NONE = 0xFFFFFFFF
REGION = np.dtype([("root", "<u4"), ("radius_sq", "<u4"), ("voxels", "<u4"), ("throats", "<u4"), ("lo", "<u2", (3,)), ("hi", "<u2", (3,)), ("flags", "<u4")])
THROAT = np.dtype([("a", "<u4"), ("b", "<u4"), ("faces", "<u4"), ("neck_sq", "<u4"), ("neck_voxel", "<u4")])
assert REGION.itemsize == 32 and THROAT.itemsize == 20

members = tr.members
radius = tr.radius                                                     # int64 [N, N, N]: R on members, 0 elsewhere
balls = tr.balls


def parents(R):
    """uint32 [N^3]: index(parent(v)) on members, NONE elsewhere"""
    N = R.shape[0]
    n3 = N ** 3
    flat = R.reshape(-1)
    index = np.arange(n3, dtype=np.uint64)
    keys = np.where(flat > 0, (flat.astype(np.uint64) << np.uint64(32)) | (np.uint64(NONE) - index), np.uint64(0))
    table = [keys.reshape(N, N, N)]                                    # table[j][z, y, x] = max keys[z, y, x .. x + 2^j - 1] where that fits the row
    while 2 << (len(table) - 1) <= N:
        prev, half = table[-1], 1 << (len(table) - 1)
        nxt = prev.copy()
        nxt[..., :N - half] = np.maximum(prev[..., :N - half], prev[..., half:])
        table.append(nxt)
    table = np.stack(table).reshape(len(table), n3)
    log2 = np.floor(np.log2(np.arange(1, N + 2))).astype(np.int64)     # log2[L - 1] = floor(log2 L)
    centres = np.flatnonzero(flat > 0)
    centres = centres[np.argsort(-flat[centres], kind="stable")]
    Rc = flat[centres]
    cz, cy, cx = centres // (N * N), centres // N % N, centres % N
    best = keys[centres].copy()
    h = int(np.sqrt(Rc[0])) if len(Rc) else 0
    while h * h > (Rc[0] if len(Rc) else 0):
        h -= 1
    for dz in range(-h, h + 1):
        for dy in range(-h, h + 1):
            d = dz * dz + dy * dy
            n = int(np.searchsorted(-Rc, -d, side="right"))           # the centres with R >= d
            if not n:
                continue
            zz, yy = cz[:n] + dz, cy[:n] + dy
            ok = (zz >= 0) & (zz < N) & (yy >= 0) & (yy < N)
            if not ok.any():
                continue
            zz, yy, xx, rest = zz[ok], yy[ok], cx[:n][ok], Rc[:n][ok] - d
            w = np.floor(np.sqrt(rest.astype(np.float64))).astype(np.int64)
            w = np.where(w * w > rest, w - 1, w)
            a, b = np.maximum(xx - w, 0), np.minimum(xx + w, N - 1)
            j = log2[b - a]
            base = (zz * N + yy) * N
            cand = np.maximum(table[j, base + a], table[j, base + b - (1 << j) + 1])
            sel = np.flatnonzero(ok)
            best[sel] = np.maximum(best[sel], cand)
    out = np.full(n3, NONE, np.uint32)
    out[centres] = (np.uint64(NONE) - (best & np.uint64(NONE))).astype(np.uint32)
    return out


def roots(parent):
    """uint32 [N^3]: index(root(v)) on members, NONE elsewhere -- by pointer jumping"""
    n3 = len(parent)
    member = parent != NONE
    up = np.where(member, parent, np.arange(n3, dtype=np.uint32)).astype(np.int64)
    while True:
        nxt = up[up]
        if np.array_equal(nxt, up):
            break
        up = nxt
    return np.where(member, up, NONE).astype(np.uint32)


def partition(grid, of, cap_sq, want_throats=True):
    """(labels uint32 [N, N, N], table REGION [K], throats THROAT [T]), form (a)"""
    R = radius(grid, of, cap_sq)
    N = R.shape[0]
    root = roots(parents(R))
    member = root != NONE
    which, inverse = np.unique(root[member], return_inverse=True)     # ascending index(root)
    K = len(which)
    labels = np.zeros(N ** 3, np.uint32)
    labels[member] = inverse.reshape(-1) + 1
    table = np.zeros(K, REGION)
    table["root"] = which
    table["radius_sq"] = R.reshape(-1)[which]
    own = labels[member].astype(np.int64) - 1
    table["voxels"] = np.bincount(own, minlength=K)
    at = np.flatnonzero(member)
    coords = (at % N, at // N % N, at // (N * N))
    lo, hi = np.full((K, 3), 0xFFFF, np.int64), np.zeros((K, 3), np.int64)
    border = np.zeros(K, np.int64)
    for k, c in enumerate(coords):
        np.minimum.at(lo[:, k], own, c)
        np.maximum.at(hi[:, k], own, c)
        np.maximum.at(border, own, ((c == 0) | (c == N - 1)).astype(np.int64))
    table["lo"], table["hi"], table["flags"] = lo, hi, border
    labels = labels.reshape(N, N, N)
    throats = np.zeros(0, THROAT)
    if want_throats and K:
        index = np.arange(N ** 3, dtype=np.int64).reshape(N, N, N)
        found = []
        for axis in range(3):
            p = tuple(slice(0, N - 1) if k == axis else slice(None) for k in range(3))
            q = tuple(slice(1, N) if k == axis else slice(None) for k in range(3))
            la, lb = labels[p].astype(np.int64), labels[q].astype(np.int64)
            m = (la > 0) & (lb > 0) & (la != lb)
            found.append(np.stack([np.minimum(la, lb)[m], np.maximum(la, lb)[m], np.minimum(R[p], R[q])[m], index[p][m]]))
        a, b, neck, voxel = np.concatenate(found, axis=1)
        pairs, inv, count = np.unique((a << 32) | b, return_inverse=True, return_counts=True)
        inv = inv.reshape(-1)
        throats = np.zeros(len(pairs), THROAT)
        throats["a"], throats["b"], throats["faces"] = pairs >> 32, pairs & 0xFFFFFFFF, count
        widest = np.zeros(len(pairs), np.int64)
        np.maximum.at(widest, inv, neck)
        first = np.full(len(pairs), N ** 3, np.int64)
        attains = neck == widest[inv]
        np.minimum.at(first, inv[attains], voxel[attains])
        throats["neck_sq"], throats["neck_voxel"] = widest, first
        table["throats"] = np.bincount(throats["a"].astype(np.int64) - 1, minlength=K) + np.bincount(throats["b"].astype(np.int64) - 1, minlength=K)
    return labels, table, throats


def partition_literal(grid, of, cap_sq):
    """(labels, table, throats, parent uint32 [N^3]), form (b): the definition, voxel by voxel; small grids only"""
    R = radius(grid, of, cap_sq)
    N = R.shape[0]
    assert N <= 12
    voxels = [(z, y, x) for z in range(N) for y in range(N) for x in range(N)]
    index = {v: (v[0] * N + v[1]) * N + v[2] for v in voxels}
    rank = {v: (int(R[v]), -index[v]) for v in voxels}                 # u above v iff rank[u] > rank[v]
    parent = {}
    for c in voxels:
        if R[c]:
            ball = [u for u in voxels if (u[0] - c[0]) ** 2 + (u[1] - c[1]) ** 2 + (u[2] - c[2]) ** 2 <= R[c]]
            parent[c] = max(ball, key=lambda u: rank[u])
    root = {}
    for c in parent:
        u = c
        while parent[u] != u:
            assert rank[parent[u]] > rank[u]
            u = parent[u]
        root[c] = u
    number = {r: k + 1 for k, r in enumerate(sorted(set(root.values()), key=lambda u: index[u]))}
    labels = np.zeros((N, N, N), np.uint32)
    table = np.zeros(len(number), REGION)
    table["lo"] = 0xFFFF
    for c, r in root.items():
        k = number[r]
        labels[c] = k
        rec = table[k - 1]
        rec["root"], rec["radius_sq"] = index[r], R[r]
        rec["voxels"] += 1
        for axis, coord in enumerate((c[2], c[1], c[0])):
            rec["lo"][axis] = min(rec["lo"][axis], coord)
            rec["hi"][axis] = max(rec["hi"][axis], coord)
            if coord in (0, N - 1):
                rec["flags"] = 1
    met = {}
    for p in voxels:
        for e in ((0, 0, 1), (0, 1, 0), (1, 0, 0)):
            q = (p[0] + e[0], p[1] + e[1], p[2] + e[2])
            if max(q) < N and labels[p] and labels[q] and labels[p] != labels[q]:
                pair = (min(int(labels[p]), int(labels[q])), max(int(labels[p]), int(labels[q])))
                met.setdefault(pair, []).append((min(int(R[p]), int(R[q])), index[p]))
    throats = np.zeros(len(met), THROAT)
    for t, pair in enumerate(sorted(met)):
        neck = max(n for n, _ in met[pair])
        throats[t] = (pair[0], pair[1], len(met[pair]), neck, min(v for n, v in met[pair] if n == neck))
        table["throats"][pair[0] - 1] += 1
        table["throats"][pair[1] - 1] += 1
    flat = np.full(N ** 3, NONE, np.uint32)
    for c, u in parent.items():
        flat[index[c]] = index[u]
    return labels, table, throats, flat


def pore_network(table, throats):
    """the restated twin of dxrvoxelizer_amd.pore_network"""
    table, throats = np.asarray(table), np.asarray(throats)
    return {"radius": np.sqrt(table["radius_sq"].astype(np.float64)), "voxels": table["voxels"].astype(np.int64), "coordination": table["throats"].astype(np.int64),
            "pairs": np.stack([throats["a"], throats["b"]], axis=1).astype(np.int64) if len(throats) else np.zeros((0, 2), np.int64),
            "neck_radius": np.sqrt(throats["neck_sq"].astype(np.float64)), "faces": throats["faces"].astype(np.int64)}


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


# ---- the grids of the tests -----------------------------------------------------------------------------------------------------------------
def dumbbell():
    """32^3: balls of radius 7 and 6 on a bar of radius 2 along x"""
    z, y, x = np.indices((32, 32, 32))
    g = (z - 16) ** 2 + (y - 16) ** 2 + (x - 9) ** 2 <= 49
    g |= (z - 16) ** 2 + (y - 16) ** 2 + (x - 23) ** 2 <= 36
    g |= ((z - 16) ** 2 + (y - 16) ** 2 <= 4) & (x >= 9) & (x <= 23)
    return g.astype(np.uint8)


def torus(N=32, major=9.0, minor=3.0):
    z, y, x = np.indices((N, N, N))
    c = (N - 1) / 2.0
    ring = np.sqrt((y - c) ** 2 + (x - c) ** 2) - major
    return (ring ** 2 + (z - c) ** 2 <= minor ** 2).astype(np.uint8)


def sheet(N):
    """a plate one voxel thick"""
    g = np.zeros((N, N, N), np.uint8)
    g[N // 2] = 1
    return g


def rod(N):
    """a rod one voxel wide along x"""
    g = np.zeros((N, N, N), np.uint8)
    g[N // 2, N // 2 - 1, :] = 1
    return g


def noise(N, density, seed):
    return (np.random.default_rng(seed).random((N, N, N)) < density).astype(np.uint8)


def ball_beside_blobs():
    """72^3: one ball of radius 30 off the middle -- its reach crosses the grid's edge -- beside five small balls"""
    z, y, x = np.indices((72, 72, 72))
    g = (z - 33) ** 2 + (y - 36) ** 2 + (x - 50) ** 2 <= 900
    return (g | (balls(72, 11, count=5, rmax=9) != 0)).astype(np.uint8)
