"""Numpy restatement of the sparse voxel octree rule (include/dxv.h: dxv_octree), written from the rule's text: a pyramid of
cell states by reshapes, one node per mixed cell and the root, levels one after another, ascending Morton code inside a level.  No dense
scan, no bricks: none of the kernels' steps."""
import numpy as np

EMPTY, FULL, MIXED = 0, 1, 2


def levels_of(N):
    L = 1
    while (1 << L) < N:
        L += 1
    return L


def morton(x, y, z, bits):
    """Morton code of cell positions: per bit triple x is the lowest bit, then y, then z"""
    code = np.zeros(np.shape(x), np.uint64)
    for b in range(bits):
        code |= ((x >> b & 1).astype(np.uint64) << np.uint64(3 * b)) | ((y >> b & 1).astype(np.uint64) << np.uint64(3 * b + 1)) \
            | ((z >> b & 1).astype(np.uint64) << np.uint64(3 * b + 2))
    return code


def children(a):
    """[s, s, s] (z, y, x) of level l + 1 -> [8, s/2, s/2, s/2]: child o = dx | dy << 1 | dz << 2 of every cell of level l"""
    return np.stack([a[(o >> 2 & 1)::2, (o >> 1 & 1)::2, (o & 1)::2] for o in range(8)])


def build(grid):
    """(nodes [n, 2] uint32 {word0, word1}, level_first [L + 1]) of a uint8 [N, N, N] grid (z, y, x)"""
    grid = np.asarray(grid)
    N = grid.shape[0]
    assert grid.shape == (N, N, N) and N % 2 == 0 and 2 <= N <= 2048
    L = levels_of(N)
    S = 1 << L
    state = np.zeros((S, S, S), np.uint8)                               # voxels of the cube outside the grid are empty
    state[:N, :N, :N] = np.where(grid != 0, FULL, EMPTY)
    mixed, full = [None] * L, [None] * L                                # per level 0 .. L - 1: the two bytes of word1 of every cell
    states = [None] * L
    for l in range(L - 1, -1, -1):
        c = children(state)
        mixed[l] = sum(((c[o] == MIXED).astype(np.uint32) << o) for o in range(8))
        full[l] = sum(((c[o] == FULL).astype(np.uint32) << o) for o in range(8))
        state = np.where(full[l] == 0xFF, FULL, np.where((mixed[l] | full[l]) == 0, EMPTY, MIXED)).astype(np.uint8)
        states[l] = state
    # the nodes of every level: the root, and the mixed cells of levels 1 .. L - 1, in ascending Morton code
    where, index, level_first, n = [], [], [], 0
    for l in range(L):
        z, y, x = np.nonzero(states[l] == MIXED) if l else (np.zeros(1, np.int64),) * 3
        order = np.argsort(morton(x, y, z, l), kind="stable")
        z, y, x = z[order], y[order], x[order]
        idx = np.full(states[l].shape, -1, np.int64)
        idx[z, y, x] = n + np.arange(len(x))
        where.append((z, y, x))
        index.append(idx)
        level_first.append(n)
        n += len(x)
    level_first.append(n)
    nodes = np.zeros((n, 2), np.uint32)
    for l in range(L):
        z, y, x = where[l]
        m = mixed[l][z, y, x]
        nodes[level_first[l]:level_first[l + 1], 1] = m | full[l][z, y, x] << 8
        has = m != 0
        if has.any():
            assert l + 1 < L                                            # at level L - 1 the children are voxels: none is mixed
            low = np.zeros(len(m), np.int64)                            # the lowest-numbered mixed child
            for o in range(7, -1, -1):
                low = np.where(m >> o & 1, o, low)
            child = index[l + 1][2 * z + (low >> 2 & 1), 2 * y + (low >> 1 & 1), 2 * x + (low & 1)]
            assert (child[has] >= 0).all()
            nodes[level_first[l]:level_first[l + 1], 0] = np.where(has, child, 0)
    return nodes, level_first


def popcount8(v):
    return sum((v >> b & 1) for b in range(8))


def expand(nodes, levels, N):
    """uint8 [N, N, N] of 0 / 1 from a well-formed tree, level by level from the root"""
    nodes = np.asarray(nodes, np.uint32).reshape(-1, 2)
    node = np.zeros((1, 1, 1), np.int64)                                # the node of every mixed cell of the level, -1 elsewhere
    solid = np.zeros((1, 1, 1), bool)                                   # cells that lie inside a full cell
    for l in range(levels):
        s = 2 << l
        nxt, sol = np.full((s, s, s), -1, np.int64), np.zeros((s, s, s), bool)
        live = node >= 0
        w0, w1 = nodes[np.where(live, node, 0), 0].astype(np.int64), nodes[np.where(live, node, 0), 1].astype(np.int64)
        for o in range(8):
            sl = (slice(o >> 2 & 1, None, 2), slice(o >> 1 & 1, None, 2), slice(o & 1, None, 2))
            sol[sl] = solid | (live & ((w1 >> (8 + o) & 1) != 0))
            nxt[sl] = np.where(live & ((w1 >> o & 1) != 0), w0 + popcount8(w1 & ((1 << o) - 1)), -1)
        node, solid = nxt, sol
    assert (node < 0).all()
    return solid[:N, :N, :N].astype(np.uint8)


def ball(N, r=None):
    z, y, x = np.indices((N, N, N))
    c, r = (N - 1) / 2, (0.4 * N if r is None else r)
    return ((x - c) ** 2 + (y - c) ** 2 + (z - c) ** 2 <= r * r).astype(np.uint8)


def shell(N):
    """a one-voxel-thick shell: the ball's voxels with an empty 6-neighbour (or on the grid's border)"""
    b = np.pad(ball(N), 1).astype(bool)
    inner = b[1:-1, 1:-1, 1:-1]
    allnb = b[:-2, 1:-1, 1:-1] & b[2:, 1:-1, 1:-1] & b[1:-1, :-2, 1:-1] & b[1:-1, 2:, 1:-1] & b[1:-1, 1:-1, :-2] & b[1:-1, 1:-1, 2:]
    return (inner & ~allnb).astype(np.uint8)


def rule_grids(N, seed=11):
    """(name, grid) of the rule tests at side N: random at two densities, a checkerboard, a solid ball, a one-voxel-thick shell"""
    rng = np.random.default_rng(seed + N)
    z, y, x = np.indices((N, N, N))
    yield f"random 0.5 {N}", (rng.random((N, N, N)) < 0.5).astype(np.uint8) * 0xFF
    yield f"random 0.02 {N}", (rng.random((N, N, N)) < 0.02).astype(np.uint8)
    yield f"checkerboard {N}", ((x + y + z) & 1).astype(np.uint8)
    yield f"ball {N}", ball(N)
    yield f"shell {N}", shell(N)
