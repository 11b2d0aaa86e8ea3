"""Two numpy restatements of the skeleton graph's rule (include/dxv.h, "Skeleton graph"), written from the rule alone and sharing no counting:
(a) `by_sets`: 27-point sums for deg, scipy.ndimage.label with the full 3x3x3 structure for the numbering, steps and attachments by
    shifted-mask pair counts over the 13 half offsets;
(b) `by_walk`: neighbour lists of the member voxels, nodes by flood, every branch followed voxel by voxel from a node voxel's curve neighbour
    to its other attachment, what is left over traced as cycles.
Both return (labels uint32 [N, N, N], nodes NODE [K], branches BRANCH [B]); tests/test_skeleton_restated.py holds them to one another on every
builder.  `prune` restates dxv_skeleton_prune on a grid.  A plain helper: no fixtures, no hooks."""
import itertools

import numpy as np
from scipy import ndimage

NODE = np.dtype([("first", "<u4"), ("voxels", "<u4"), ("degree", "<u4"), ("flags", "<u4"), ("lo", "<u2", 3), ("hi", "<u2", 3), ("w_max", "<u4")])
BRANCH = np.dtype([("a", "<u4"), ("b", "<u4"), ("first", "<u4"), ("voxels", "<u4"), ("steps", "<u4", 3), ("flags", "<u4"), ("w_min", "<u4"), ("w_max", "<u4"), ("w_sum", "<u8")])
assert NODE.itemsize == 32 and BRANCH.itemsize == 48
BRANCH_BIT = 0x80000000
NODE_BORDER, NODE_END, NODE_JUNCTION = 1, 2, 4
CLOSED, BORDER, SPUR = 1, 2, 4
OFFSETS = [o for o in itertools.product((-1, 0, 1), repeat=3) if o != (0, 0, 0)]          # (dz, dy, dx)
HALF = [o for o in OFFSETS if o > (0, 0, 0)]                                              # one of every pair {o, -o}: 13


def _shifted(a, o):
    """b[p] = a[p + o], zeros from outside the grid"""
    N = a.shape[0]
    out = np.zeros_like(a)
    src = tuple(slice(max(d, 0), N + min(d, 0)) for d in o)
    dst = tuple(slice(max(-d, 0), N + min(-d, 0)) for d in o)
    out[dst] = a[src]
    return out


def degree(grid):
    """int [N, N, N]: the members among the 26 neighbours, 0 off the members; by a 27-point sum"""
    m = (np.asarray(grid) != 0).astype(np.int64)
    total = ndimage.convolve(m, np.ones((3, 3, 3), np.int64), mode="constant", cval=0)
    return (total - m) * m


def voxel_counts(grid):
    """(end_voxels, curve_voxels, junction_voxels): the members with deg <= 1, == 2, >= 3"""
    m, d = np.asarray(grid) != 0, degree(grid)
    return int(np.count_nonzero(m & (d <= 1))), int(np.count_nonzero(m & (d == 2))), int(np.count_nonzero(m & (d >= 3)))


def _finish(nodes, branches, weights):
    tip = (nodes["voxels"] == 1) & (nodes["degree"] == 1)
    for r in branches:
        if r["a"] and tip[r["a"] - 1] != tip[r["b"] - 1]:
            r["flags"] |= SPUR
    if weights is None:
        for name in ("w_min", "w_max", "w_sum"):
            branches[name] = 0
        nodes["w_max"] = 0
    return nodes, branches


def by_sets(grid, weights=None):
    g = np.asarray(grid)
    N = g.shape[0]
    m, d = g != 0, degree(g)
    curve, node = m & (d == 2), m & (d != 2)
    full = np.ones((3, 3, 3), bool)
    nl, K = ndimage.label(node, full)
    bl, B = ndimage.label(curve, full)
    labels = (nl.astype(np.uint32) + np.where(bl > 0, bl.astype(np.uint32) | np.uint32(BRANCH_BIT), np.uint32(0))).astype(np.uint32)
    index = np.arange(N ** 3, dtype=np.int64).reshape(N, N, N)
    z, y, x = np.indices((N, N, N))
    border = (x == 0) | (x == N - 1) | (y == 0) | (y == N - 1) | (z == 0) | (z == N - 1)
    W = None if weights is None else np.asarray(weights, np.uint32).reshape(N, N, N).astype(np.uint64)
    nodes, branches = np.zeros(K, NODE), np.zeros(B, BRANCH)
    for table, lab, count in ((nodes, nl, K), (branches, bl, B)):
        if not count:
            continue
        sel = lab > 0
        ids = lab[sel] - 1
        table["voxels"] = np.bincount(ids, minlength=count)
        first = np.full(count, N ** 3, np.int64)
        np.minimum.at(first, ids, index[sel])
        table["first"] = first
    if K:
        sel = nl > 0
        ids = nl[sel] - 1
        for axis, coord in enumerate((x, y, z)):
            lo, hi = np.full(K, N, np.int64), np.zeros(K, np.int64)
            np.minimum.at(lo, ids, coord[sel])
            np.maximum.at(hi, ids, coord[sel])
            nodes["lo"][:, axis], nodes["hi"][:, axis] = lo, hi
        for bit, what in ((NODE_BORDER, border), (NODE_END, d <= 1), (NODE_JUNCTION, d >= 3)):
            nodes["flags"] |= (np.bincount(ids, weights=what[sel], minlength=K) > 0).astype(np.uint32) * np.uint32(bit)
        if W is not None:
            wmax = np.zeros(K, np.uint64)
            np.maximum.at(wmax, ids, W[sel])
            nodes["w_max"] = wmax
    if B:
        sel = bl > 0
        ids = bl[sel] - 1
        branches["flags"] |= (np.bincount(ids, weights=border[sel], minlength=B) > 0).astype(np.uint32) * np.uint32(BORDER)
        if W is not None:
            wmin, wmax, wsum = np.full(B, 0xFFFFFFFF, np.uint64), np.zeros(B, np.uint64), np.zeros(B, np.uint64)
            np.minimum.at(wmin, ids, W[sel])
            np.maximum.at(wmax, ids, W[sel])
            np.add.at(wsum, ids, W[sel])
            branches["w_min"], branches["w_max"], branches["w_sum"] = wmin, wmax, wsum
        a, b = np.full(B, 0xFFFFFFFF, np.int64), np.zeros(B, np.int64)
        steps = np.zeros((B, 3), np.int64)
        deg = np.zeros(K + 1, np.int64)
        for o in HALF:
            t = sum(1 for c in o if c) - 1
            mq, cq, blq, nlq = (_shifted(v, o) for v in (m, curve, bl, nl))
            pair = m & mq & (curve | cq)
            owner = np.where(curve, bl, blq)[pair] - 1                  # the branch of its curve voxel(s): adjacent curve voxels share it
            np.add.at(steps[:, t], owner, 1)
            for att, who in ((pair & curve & ~cq, nlq), (pair & cq & ~curve, nl)):     # the other voxel is a node voxel
                br, nd = np.where(curve, bl, blq)[att] - 1, who[att]
                np.minimum.at(a, br, nd)
                np.maximum.at(b, br, nd)
                np.add.at(deg, nd, 1)
        closed = b == 0
        branches["a"], branches["b"] = np.where(closed, 0, a), b
        branches["flags"] |= closed.astype(np.uint32) * np.uint32(CLOSED)
        branches["steps"] = steps
        nodes["degree"] = deg[1:]
    nodes, branches = _finish(nodes, branches, weights)
    return labels, nodes, branches


def by_walk(grid, weights=None):
    g = np.asarray(grid)
    N = g.shape[0]
    W = None if weights is None else np.asarray(weights, np.uint32).reshape(-1)
    members = [tuple(int(c) for c in p) for p in np.argwhere(g != 0)]                     # ascending index
    inside = set(members)
    nbrs = {p: [q for q in ((p[0] + o[0], p[1] + o[1], p[2] + o[2]) for o in OFFSETS) if q in inside] for p in members}
    idx = lambda p: (p[0] * N + p[1]) * N + p[2]
    on_border = lambda p: any(c == 0 or c == N - 1 for c in p)
    step_type = lambda p, q: sum(1 for u, v in zip(p, q) if u != v) - 1
    is_curve = {p: len(nbrs[p]) == 2 for p in members}
    labels = np.zeros(N ** 3, np.uint32)
    node_of, node_rows = {}, []
    for p in members:                                                   # nodes by flood, in ascending order of their first voxel
        if is_curve[p] or p in node_of:
            continue
        k = len(node_rows) + 1
        todo, cluster = [p], [p]
        node_of[p] = k
        while todo:
            u = todo.pop()
            for q in nbrs[u]:
                if not is_curve[q] and q not in node_of:
                    node_of[q] = k
                    todo.append(q)
                    cluster.append(q)
        node_rows.append(cluster)
    found, seen = [], set()                                             # (voxels, attached node numbers, steps[3])

    def follow(prev, cur, attached, steps):
        path = [cur]
        seen.add(cur)
        while True:
            nxt = [q for q in nbrs[cur] if q != prev]
            assert len(nxt) == 1
            nxt = nxt[0]
            steps[step_type(cur, nxt)] += 1
            if not is_curve[nxt]:
                attached.append(node_of[nxt])
                return path
            if nxt in seen:                                             # a cycle closed on its first voxel
                return path
            prev, cur = cur, nxt
            path.append(cur)
            seen.add(cur)

    for p in members:                                                   # the paths: from every node voxel's curve neighbour to the other attachment
        if is_curve[p]:
            continue
        for c in nbrs[p]:
            if is_curve[c] and c not in seen:
                attached, steps = [node_of[p]], [0, 0, 0]
                steps[step_type(p, c)] += 1
                found.append((follow(p, c, attached, steps), attached, steps))
    for p in members:                                                   # what is left over: cycles
        if is_curve[p] and p not in seen:
            steps = [0, 0, 0]
            found.append((follow(nbrs[p][0], p, [], steps), [], steps))
    found.sort(key=lambda f: min(idx(v) for v in f[0]))
    nodes, branches = np.zeros(len(node_rows), NODE), np.zeros(len(found), BRANCH)
    for k, cluster in enumerate(node_rows):
        r = nodes[k]
        r["first"], r["voxels"] = min(idx(v) for v in cluster), len(cluster)
        for axis in range(3):                                           # (x, y, z) from (z, y, x)
            r["lo"][axis], r["hi"][axis] = min(v[2 - axis] for v in cluster), max(v[2 - axis] for v in cluster)
        r["flags"] = ((NODE_BORDER if any(on_border(v) for v in cluster) else 0) | (NODE_END if any(len(nbrs[v]) <= 1 for v in cluster) else 0) |
                      (NODE_JUNCTION if any(len(nbrs[v]) >= 3 for v in cluster) else 0))
        if W is not None:
            r["w_max"] = max(int(W[idx(v)]) for v in cluster)
        for v in cluster:
            labels[idx(v)] = k + 1
    for b, (path, attached, steps) in enumerate(found):
        r = branches[b]
        assert len(attached) in (0, 2) and sum(steps) == len(path) + (1 if attached else 0) and (attached or len(path) >= 3)
        r["a"], r["b"] = (min(attached), max(attached)) if attached else (0, 0)
        r["first"], r["voxels"], r["steps"] = min(idx(v) for v in path), len(path), steps
        r["flags"] = (0 if attached else CLOSED) | (BORDER if any(on_border(v) for v in path) else 0)
        for k in attached:
            nodes[k - 1]["degree"] += 1
        if W is not None:
            w = [int(W[idx(v)]) for v in path]
            r["w_min"], r["w_max"], r["w_sum"] = min(w), max(w), sum(w)
        for v in path:
            labels[idx(v)] = BRANCH_BIT | (b + 1)
    nodes, branches = _finish(nodes, branches, weights)
    return labels.reshape(N, N, N), nodes, branches


def len345(branches):
    s = branches["steps"].astype(np.int64)
    return 3 * s[:, 0] + 4 * s[:, 1] + 5 * s[:, 2]


def prune(grid, max_len345):
    """(grid after dxv_skeleton_prune(max_len345), branches removed, voxels removed): every spur at or below the bound goes with its tip, in one
    pass; every other byte stays as it is"""
    g = np.array(grid, np.uint8)
    labels, nodes, branches = by_sets(g)
    goes = ((branches["flags"] & SPUR) != 0) & (len345(branches) <= max_len345)
    tip = (nodes["voxels"] == 1) & (nodes["degree"] == 1)
    removed = 0
    for b in np.flatnonzero(goes):
        r = branches[b]
        k = r["a"] if tip[r["a"] - 1] else r["b"]
        sel = (labels == (BRANCH_BIT | (b + 1))) | (labels == k)
        removed += int(np.count_nonzero(sel))
        g[sel] = 0
    return g, int(np.count_nonzero(goes)), removed


# ---- the builders: the figures of tests/test_gpu_skeleton.py, each a (name, uint8 [N, N, N]) ------------------------------------------------
def _grid(N, voxels, value=1):
    g = np.zeros((N, N, N), np.uint8)
    for z, y, x in voxels:
        g[z, y, x] = value
    return g


def diamond(c=8, r=4, z=8):
    """a closed ring of diagonal steps in the plane z: every voxel has deg 2"""
    return [(z, c + dy, c + dx) for dy in range(-r, r + 1) for dx in range(-r, r + 1) if abs(dy) + abs(dx) == r]


def figures(N=16):
    h = N // 2
    seg = lambda d, n=6: [(h + d[0] * k, h + d[1] * k, h + d[2] * k) for k in range(-(n // 2), n - n // 2)]
    ring = [(h, y, x) for y in range(4, 11) for x in range(4, 11) if y in (4, 10) or x in (4, 10)]
    y_fig = [(h, h, x) for x in range(3, h + 1)] + [(h, h - k, h + k) for k in range(1, 3)] + [(h, h + k, h + k) for k in range(1, 6)]
    theta = ([(h, 8, x) for x in range(4, 13)] + [(h, 9, 5), (h, 10, 6), (h, 10, 7), (h, 10, 8), (h, 10, 9), (h, 10, 10), (h, 9, 11)] +
             [(h + 1, 7, 5), (h + 2, 6, 6), (h + 2, 6, 7), (h + 2, 6, 8), (h + 2, 6, 9), (h + 2, 6, 10), (h + 1, 7, 11)])
    out = [("single voxel", _grid(N, [(h, h, h)], 0xFF)), ("two voxels", _grid(N, [(h, h, h), (h, h + 1, h + 1)], 2)),
           ("segment x", _grid(N, seg((0, 0, 1)))), ("segment y", _grid(N, seg((0, 1, 0)), 7)), ("segment z", _grid(N, seg((1, 0, 0)))),
           ("plane diagonal", _grid(N, seg((0, 1, 1)))), ("space diagonal", _grid(N, seg((1, 1, -1)), 0x80)),
           ("three mutually adjacent", _grid(N, [(h, h, h), (h, h, h + 1), (h, h + 1, h)])), ("Y", _grid(N, y_fig)), ("theta", _grid(N, theta)),
           ("loop at one node", _grid(N, diamond(8, 4, h) + [(h, 8, 13), (h, 8, 14)])), ("closed diamond", _grid(N, diamond(8, 4, h), 3)),
           ("square ring", _grid(N, ring))]
    for name, g in list(out):
        for corner in (0, 1):
            out.append((f"{name}, at corner {corner}", pushed(g, corner)))
    out += [("empty", np.zeros((N, N, N), np.uint8)), ("all 0xFF", np.full((N, N, N), 0xFF, np.uint8))]
    return out


def pushed(g, corner):
    """the figure moved until its box touches the grid's corner 0 or corner N - 1"""
    N = g.shape[0]
    at = np.argwhere(g != 0)
    lo, hi = at.min(axis=0), at.max(axis=0)
    box = g[lo[0]:hi[0] + 1, lo[1]:hi[1] + 1, lo[2]:hi[2] + 1]
    out = np.zeros_like(g)
    s = [slice(0, n) if corner == 0 else slice(N - n, N) for n in box.shape]
    out[s[0], s[1], s[2]] = box
    return out


def seams(N):
    """figures across the word seam x = 63 | 64 of a row of N > 64 voxels, and on the row's last bit"""
    h = N // 2
    across = _grid(N, [(h, h, x) for x in range(58, 70)])
    cluster = _grid(N, [(h, h, x) for x in range(56, 72)] + [(h, h + 1, 63), (h, h + 1, 64), (h, h - 1, 63), (h, h - 1, 64), (h + 1, h, 63), (h + 1, h, 64)] +
                    [(h, h + 1 + k, 64 + k) for k in range(1, 5)])
    last = _grid(N, [(h, h, x) for x in range(N - 7, N)] + [(1, k, N - 1 - k) for k in range(5)], 0x40)
    diag = _grid(N, [(h, 60 + k, 60 + k) for k in range(9) if 60 + k < N] + [(h + 1 + k, 68, 68 - k) for k in range(1, 6)])
    return [("branch across the seam", across), ("node cluster on the seam", cluster), ("branch to the row's last bit", last), ("diagonals across the seam", diag)]


def random_grid(N, density, seed):
    rng = np.random.default_rng(seed)
    return ((rng.random((N, N, N)) < density) * rng.integers(1, 256, (N, N, N))).astype(np.uint8)


def contended(N=32):
    """one-voxel nodes and three-voxel branches, thousands of them: K and B are large against the voxel count"""
    g = np.zeros((N, N, N), np.uint8)
    h = N // 2
    g[0:h - 1:2, 0::2, 0::2] = 1                                        # isolated voxels, two apart: one-voxel nodes
    for dy, dx in ((0, 0), (0, 1), (1, 0)):                             # three mutually adjacent voxels, four apart: closed branches of three
        g[h:N - 8:2, dy::4, dx::4] = 1
    for x in (0, 1, 2):                                                 # three voxels in a row: two tips and a one-voxel branch between them
        g[N - 7::2, 0::2, x::4] = 1
    return g


def builders():
    out = figures(16)
    for N in (72, 130):
        out += [(f"{name}, N = {N}", g) for name, g in seams(N)]
    out += [(f"random {density} at {N}", random_grid(N, density, 7 * N + int(100 * density))) for N in (12, 16, 24) for density in (0.03, 0.1, 0.2)]
    out.append(("contended", contended(32)))
    return out
