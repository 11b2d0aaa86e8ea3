"""Topology-preserving thinning restated in numpy, from the rule's text alone (include/dxv.h over dxv_thin_async):

    solid(p)     byte(p) != 0; voxels outside the grid are EMPTY
    T26(p)       the 26-connected components of the solid voxels of N26*(p)
    T6(p)        the 6-connected components of the empty voxels of N18*(p) that contain a voxel of N6*(p)
    simple(p)    T26(p) == 1 and T6(p) == 1
    iteration    B = the solid voxels with an empty face neighbour, as they are at its start; then for s = 0 .. 7 every p of B that is still
                 solid, has (x & 1) | (y & 1) << 1 | (z & 1) << 2 == s, is simple in the current set and is not kept by the kind goes, all at once
    kinds        CURVE keeps p when exactly one voxel of N26*(p) is solid; KERNEL keeps nothing
    stopping     an iteration that removes nothing is the confirming one; or max_iterations of them have run (0: no bound)

Vectorised over an iteration's candidates: their neighbourhoods are gathered into one uint32 each (bit k = the k-th of the 27 offsets in
z, y, x order, the voxel itself left out), the DISTINCT words are decided, and the decision of a word is remembered for the rest of the run.
A word is decided by its two counts, and a count by a flood inside the neighbourhood through explicit adjacency lists -- who is next to whom
is worked out from the offsets' coordinates, not from bit patterns.  No scipy."""
import numpy as np

import components_restated as cr

CURVE, KERNEL = 0, 1
KINDS = (CURVE, KERNEL)

OFFSETS = [(dz, dy, dx) for dz in (-1, 0, 1) for dy in (-1, 0, 1) for dx in (-1, 0, 1)]
CENTRE = OFFSETS.index((0, 0, 0))
_DIST = [abs(dz) + abs(dy) + abs(dx) for dz, dy, dx in OFFSETS]
N26 = sum(1 << k for k in range(27) if k != CENTRE)
N18 = sum(1 << k for k in range(27) if 1 <= _DIST[k] <= 2)
N6 = sum(1 << k for k in range(27) if _DIST[k] == 1)


def _adjacent(connectivity):
    """adj[k]: the offsets (as a bit set, the centre left out) adjacent to offset k"""
    adj = []
    for a in OFFSETS:
        m = 0
        for k, b in enumerate(OFFSETS):
            d = [abs(u - v) for u, v in zip(a, b)]
            if k != CENTRE and a != b and max(d) <= 1 and (connectivity == 26 or sum(d) == 1):
                m |= 1 << k
        adj.append(m)
    return adj


ADJ26, ADJ6 = _adjacent(26), _adjacent(6)


def _flood(seed, within, adj):
    """arrays of bit sets: the members of `within` that paths through `within` join to `seed`"""
    r = seed & within
    while True:
        n = r.copy()
        for k in range(27):
            if k != CENTRE:
                n |= np.where((r >> np.uint32(k)) & np.uint32(1), np.uint32(adj[k]), np.uint32(0))
        n &= within
        if np.array_equal(n, r):
            return r
        r = n


def _count(members, seeds, adj):
    """arrays: the components of `members` that hold a bit of `seeds`"""
    left = (seeds & members).copy()
    count = np.zeros(left.shape, np.uint32)
    while left.any():
        low = left & (~left + np.uint32(1))
        left &= ~_flood(low, members, adj)
        count += (low != 0)
    return count


def T26(cfg):
    cfg = np.asarray(cfg, np.uint32)
    solid = cfg & np.uint32(N26)
    return _count(solid, solid, ADJ26)


def T6(cfg):
    cfg = np.asarray(cfg, np.uint32)
    empty = ~cfg & np.uint32(N18)
    return _count(empty, empty & np.uint32(N6), ADJ6)


def simple(cfg):
    return (T26(cfg) == 1) & (T6(cfg) == 1)


def popcount(cfg):
    cfg = np.asarray(cfg, np.uint32)
    return sum(((cfg >> np.uint32(k)) & np.uint32(1)).astype(np.uint32) for k in range(27))


def removes(cfg, kind):
    cfg = np.asarray(cfg, np.uint32) & np.uint32(N26)
    out = simple(cfg)
    if kind == CURVE:
        out &= popcount(cfg) != 1
    return out


class _Decisions:
    """configuration -> removed or not under either kind (bit `kind` of a byte), decided once per distinct word for the whole process: a verdict
    depends on the word alone"""

    def __init__(self):
        self.known = np.zeros(0, np.uint32)
        self.verdict = np.zeros(0, np.uint8)

    def __call__(self, cfg, kind):
        distinct = np.unique(cfg)
        new = np.setdiff1d(distinct, self.known, assume_unique=True)
        if len(new):
            plain = simple(new)
            both = (plain & (popcount(new) != 1)).astype(np.uint8) << CURVE | plain.astype(np.uint8) << KERNEL
            known = np.concatenate([self.known, new])
            verdict = np.concatenate([self.verdict, both])
            order = np.argsort(known)
            self.known, self.verdict = known[order], verdict[order]
        return (self.verdict[np.searchsorted(self.known, cfg)] >> kind & 1) != 0


_DECIDE = _Decisions()


def thin(grid, kind, max_iterations=0):
    """(uint8 [N, N, N] of 0 / 1, iterations run -- the confirming one included --, voxels removed, converged)"""
    assert kind in KINDS
    g = np.asarray(grid)
    N = g.shape[0]
    assert g.shape == (N, N, N)
    P = N + 2
    S = np.zeros((P, P, P), bool)                                      # one empty layer round the grid
    S[1:-1, 1:-1, 1:-1] = g != 0
    flat = S.reshape(-1)
    step = [(dz * P + dy) * P + dx for dz, dy, dx in OFFSETS]
    z, y, x = np.indices((P, P, P), sparse=True)
    sub = (((x - 1) & 1) | (((y - 1) & 1) << 1) | (((z - 1) & 1) << 2)).astype(np.uint8)
    iterations = removed = 0
    converged = False
    faces = [step[OFFSETS.index(o)] for o in OFFSETS if sum(map(abs, o)) == 1]
    sub = sub.reshape(-1)
    inner = S[1:-1, 1:-1, 1:-1]
    all_faces = S[:-2, 1:-1, 1:-1] & S[2:, 1:-1, 1:-1] & S[1:-1, :-2, 1:-1] & S[1:-1, 2:, 1:-1] & S[1:-1, 1:-1, :-2] & S[1:-1, 1:-1, 2:]
    B = np.zeros((P, P, P), bool)
    B[1:-1, 1:-1, 1:-1] = inner & ~all_faces
    border = np.flatnonzero(B)                                          # the solid voxels with an empty face neighbour, ascending
    while not max_iterations or iterations < max_iterations:
        iterations += 1
        which = sub[border]
        went = []
        for s in range(8):
            at = border[which == s]
            at = at[flat[at]]
            if not len(at):
                continue
            cfg = np.zeros(len(at), np.uint32)
            for k in range(27):
                if k != CENTRE:
                    cfg |= flat[at + step[k]].astype(np.uint32) << np.uint32(k)
            out = at[_DECIDE(cfg, kind)]
            flat[out] = False
            went.append(out)
        gone = sum(len(w) for w in went)
        removed += gone
        if not gone:
            converged = True
            break
        # the next iteration's border, without another pass over the grid: a solid voxel has an empty face neighbour then iff it has one now
        # (it is in this border and still solid) or one of its face neighbours went in this iteration
        went = np.concatenate(went)
        near = np.concatenate([went + f for f in faces] + [border])
        border = np.unique(near[flat[near]])
    return S[1:-1, 1:-1, 1:-1].astype(np.uint8), iterations, removed, converged


def counts(before, after):
    """voxels removed: what dxv_thin_info reports beside the iterations"""
    return int(np.count_nonzero((np.asarray(before) != 0) & (np.asarray(after) == 0)))


def euler(grid):
    """V - E + F - C of the complex of closed unit cubes of the solid voxels: its cells are the cubes and every face, edge and corner of one.
    A cell that extends along an axis lies in one voxel along that axis, one that does not is shared by two; it exists iff one of them is solid."""
    s = np.pad(np.asarray(grid) != 0, 1)
    n = s.shape[0] - 1
    total = 0
    for ez in (0, 1):
        for ey in (0, 1):
            for ex in (0, 1):
                cell = np.zeros((n, n, n), bool)
                for oz in range(2 - ez):
                    for oy in range(2 - ey):
                        for ox in range(2 - ex):
                            cell |= s[oz:oz + n, oy:oy + n, ox:ox + n]
                total += (-1) ** (ez + ey + ex) * int(np.count_nonzero(cell))
    return total


def topology(grid):
    """(solid 26-components, empty 6-components of the grid padded by an empty layer, Euler characteristic)"""
    padded = np.pad((np.asarray(grid) != 0).astype(np.uint8), 1)
    solid = len(np.unique(cr.firsts(padded, cr.SOLID, 26)[padded != 0]))
    empty = len(np.unique(cr.firsts(padded, cr.EMPTY, 6)[padded == 0]))
    return solid, empty, euler(grid)


def neighbours26(grid):
    """int [N, N, N]: the solid voxels among the 26 round every voxel"""
    s = np.pad((np.asarray(grid) != 0).astype(np.int32), 1)
    N = s.shape[0] - 2
    out = np.zeros((N, N, N), np.int32)
    for dz, dy, dx in OFFSETS:
        if (dz, dy, dx) != (0, 0, 0):
            out += s[1 + dz:1 + dz + N, 1 + dy:1 + dy + N, 1 + dx:1 + dx + N]
    return out


def packed_sha(grid):
    import hashlib
    return hashlib.sha256(np.packbits(np.asarray(grid).reshape(-1) != 0, bitorder="little").tobytes()).hexdigest()
