"""The integral measures of a labelling restated in numpy, from the rule's text alone (include/dxv.h over dxv_measure_async):

    record k     of component k = 1 .. K of components_restated.label(grid, of, connectivity); record 0 the sum of the others
    voxels, sum, sum2, prod   the moments of the voxel indices (x, y, z), from coordinate arrays
    faces        pairs (p, d), d one of the six axis steps, p + d a non-member or outside the grid
    euler, 26    #corners - #edges + #faces - #cubes of the closed unit cubes of the component: every lattice cell (a cube, or a face, edge or
                 corner between 2, 4 or 8 voxels) with a member round it, counted for the MAXIMUM label round it (they all have one label)
    euler, 6     voxels - 6-adjacent pairs + 2 x 2 x 1 squares - 2 x 2 x 2 blocks all of whose voxels are members, counted for the MINIMUM
                 label among them (non-zero exactly when all are members, and then they all have one label)

Cells are found per lattice cell of the whole grid and then counted per label: no ownership, no runs, no bits.  All arithmetic is exact
integer (np.add.at on int64, bincount without weights), never a float on the way.  A plain helper: no fixtures, no hooks."""
import itertools

import numpy as np

import components_restated as cr

RECORD = np.dtype([("voxels", "<u8"), ("sum", "<u8", (3,)), ("sum2", "<u8", (3,)), ("prod", "<u8", (3,)), ("faces", "<u8"), ("euler", "<i8")])
assert RECORD.itemsize == 96
_LABEL = np.uint32                                                      # labels are compared and used as indices, never added up


def _count(total, labels_of_cells, sign):
    """total[k] += sign for every cell whose label is k > 0"""
    k = labels_of_cells[labels_of_cells > 0].astype(np.int64)
    total += sign * np.bincount(k, minlength=len(total))               # (integer counts: no weights, no float)


def euler26(labels, K):
    """int64 [K + 1]: per label, the Euler characteristic of its closed unit cubes (entry 0 unused)"""
    L = np.pad(np.asarray(labels, _LABEL), 1)
    n = L.shape[0] - 1
    total = np.zeros(K + 1, np.int64)
    for ez, ey, ex in itertools.product((0, 1), repeat=3):              # 1: the cell extends along that axis and lies in one voxel along it
        cell = np.zeros((n, n, n), _LABEL)
        for oz, oy, ox in itertools.product(range(2 - ez), range(2 - ey), range(2 - ex)):
            np.maximum(cell, L[oz:oz + n, oy:oy + n, ox:ox + n], out=cell)
        # a cell that extends along an axis starts at voxel index >= 0 there: its slot 0 along that axis is the padding's and is empty anyway
        _count(total, cell, (-1) ** (ez + ey + ex))
    return total


def euler6(labels, K):
    """int64 [K + 1]: per label, voxels - pairs + squares - blocks inside it"""
    L = np.asarray(labels, _LABEL)
    N = L.shape[0]
    total = np.zeros(K + 1, np.int64)
    for ez, ey, ex in itertools.product((0, 1), repeat=3):              # 1: the cell is two voxels long along that axis
        n = (N - ez, N - ey, N - ex)
        cell = None
        for oz, oy, ox in itertools.product(range(1 + ez), range(1 + ey), range(1 + ex)):
            part = L[oz:oz + n[0], oy:oy + n[1], ox:ox + n[2]]
            cell = part.copy() if cell is None else np.minimum(cell, part)
        _count(total, cell, (-1) ** (ez + ey + ex))
    return total


def faces(labels, K):
    """int64 [K + 1]: per label, the faces of its voxels towards a non-member or the outside"""
    L = np.pad(np.asarray(labels, _LABEL), 1)
    N = L.shape[0] - 2
    mine = L[1:-1, 1:-1, 1:-1]
    total = np.zeros(K + 1, np.int64)
    for axis in range(3):
        for step in (-1, 1):
            at = [slice(1, N + 1)] * 3
            at[axis] = slice(1 + step, N + 1 + step)
            _count(total, np.where(L[tuple(at)] == 0, mine, 0), 1)
    return total


def label(grid, of=cr.SOLID, connectivity=6):
    """(labels uint32 [N, N, N], K) as components_restated.label numbers them.  Its whole-grid steps take half a minute at side 194, so where
    scipy is present its labelling is taken and numbered again by first voxel (tests/test_gpu_grid_sides.py holds the two to each other)."""
    try:
        from scipy import ndimage
    except ImportError:
        labels, table = cr.label(grid, of, connectivity)
        return labels, len(table)
    lab, K = ndimage.label(cr.members(grid, of), structure=ndimage.generate_binary_structure(3, 1 if connectivity == 6 else 3))
    values, where = np.unique(lab.ravel(), return_index=True)
    values, where = values[values > 0], where[values > 0]
    rank = np.zeros(K + 1, np.uint32)
    rank[values[np.argsort(where, kind="stable")]] = np.arange(1, K + 1, dtype=np.uint32)
    return rank[lab], K


def measure(grid, of=cr.SOLID, connectivity=6, labelling=None):
    """[K + 1] of RECORD; labelling: (labels, K) -- label(grid, of, connectivity), or cr.label's (labels, table) -- where the caller has it"""
    labels, table = label(grid, of, connectivity) if labelling is None else labelling
    K = int(table) if np.isscalar(table) else len(table)
    out = np.zeros(K + 1, RECORD)
    z, y, x = (c.astype(np.int64) for c in np.nonzero(labels))
    k = labels[labels != 0].astype(np.int64)

    def per_label(values):
        total = np.zeros(K + 1, np.int64)
        np.add.at(total, k, values)
        return total

    out["voxels"] = per_label(np.ones(len(k), np.int64))
    for a, c in enumerate((x, y, z)):
        out["sum"][:, a] = per_label(c)
        out["sum2"][:, a] = per_label(c * c)
    for a, (c, d) in enumerate(((x, y), (y, z), (z, x))):
        out["prod"][:, a] = per_label(c * d)
    out["faces"] = faces(labels, K)
    out["euler"] = euler26(labels, K) if connectivity == 26 else euler6(labels, K)
    for name in RECORD.names:
        out[name][0] = out[name][1:].sum(axis=0)
    return out


def mirrored(table, N, flips):
    """the moments of `table` as they must be for the grid flipped along the axes (x, y, z) whose entry of `flips` is true: i -> N - 1 - i"""
    out = table.copy()
    V = table["voxels"].astype(object)
    s, s2, pr = (table[n].astype(object) for n in ("sum", "sum2", "prod"))
    m = N - 1
    ns = s.copy()
    for a in range(3):
        if flips[a]:
            ns[:, a] = m * V - s[:, a]
            out["sum2"][:, a] = (m * m * V - 2 * m * s[:, a] + s2[:, a]).astype(np.uint64)
    for a in range(3):
        b = (a + 1) % 3
        p = pr[:, a]
        if flips[a] and flips[b]:
            p = m * m * V - m * s[:, a] - m * s[:, b] + p
        elif flips[a]:
            p = m * s[:, b] - p
        elif flips[b]:
            p = m * s[:, a] - p
        out["prod"][:, a] = p.astype(np.uint64)
    out["sum"] = ns.astype(np.uint64)
    return out


def permuted(table, axes):
    """the moments of `table` as they must be for the grid g.transpose(axes) (numpy axes are (z, y, x))"""
    # new numpy axis i is old numpy axis axes[i]; coordinate index a = 2 - numpy axis
    src = [2 - axes[2 - a] for a in range(3)]                           # new coordinate a is old coordinate src[a]
    out = table.copy()
    for a in range(3):
        out["sum"][:, a] = table["sum"][:, src[a]]
        out["sum2"][:, a] = table["sum2"][:, src[a]]
        pair = {src[a], src[(a + 1) % 3]}
        old = next(i for i in range(3) if {i, (i + 1) % 3} == pair)
        out["prod"][:, a] = table["prod"][:, old]
    return out
