"""Numpy restatement of the isosurface rule (include/dxv.h: dxv_isosurface), written from the rule's text: naive Surface
Nets over a float32 field of a whole N^3 grid, every operation in float32 and in the rule's order.  extract() gives the vertex and index
buffers the device must produce byte for byte; the helpers below it say what a closed, outward-oriented mesh is."""
import numpy as np

F32 = np.float32
MESH_DISTANCE, GRID_DISTANCE = 0, 1
SPACE_VOXELS, SPACE_OBJECT = 0, 1


def voxel(N, units=False):
    """P: one voxel in the field's unit -- 1 for the voxel-unit formats, 2 / N for DXV_MDIST_UNITS_F32"""
    return F32(2.0) / F32(N) if units else F32(1.0)


def extract(field, iso=0.0, P=1.0, space=SPACE_VOXELS, bound=None):
    """(vb [V, 6] float32, ib [3T] uint32) of field [N, N, N] (z, y, x)"""
    f = np.asarray(field)
    assert f.dtype == F32 and f.ndim == 3 and f.shape[0] == f.shape[1] == f.shape[2]
    N, C = f.shape[0], f.shape[0] + 1
    iso, P = F32(iso), F32(P)
    with np.errstate(all="ignore"):
        # samples -1 .. N per axis: s[k + 1, j + 1, i + 1]; outside the grid one voxel, whatever iso is
        s = np.full((N + 2,) * 3, P, F32)
        s[1:-1, 1:-1, 1:-1] = f - iso
        inside = s < 0                                                  # strictly: -0, +0 and NaN are outside

        def corner(a, arr=s):
            """the samples c - 1 + a of every cell c, [cz, cy, cx]"""
            return arr[a[2]:a[2] + C, a[1]:a[1] + C, a[0]:a[0] + C]

        corners = [(dx, dy, dz) for dz in (0, 1) for dy in (0, 1) for dx in (0, 1)]
        n_in = sum(corner(a, inside).astype(np.int32) for a in corners)
        active = (n_in != 0) & (n_in != 8)

        # the twelve edges: x, y, z; within an axis the other two offsets (0,0), (1,0), (0,1), (1,1), the lower axis first
        total = [np.zeros((C, C, C), F32) for _ in range(3)]
        g = [np.zeros((C, C, C), F32) for _ in range(3)]
        count = np.zeros((C, C, C), np.int32)
        for axis in range(3):
            lo, hi = [k for k in range(3) if k != axis]
            for d_lo, d_hi in ((0, 0), (1, 0), (0, 1), (1, 1)):
                a = [0, 0, 0]
                a[lo], a[hi] = d_lo, d_hi
                b = list(a)
                b[axis] = 1
                sa, sb = corner(a), corner(b)
                crosses = (sa < 0) != (sb < 0)
                t = np.where(np.isfinite(sa) & np.isfinite(sb), sa / (sa - sb), F32(0.5)).astype(F32)
                at = [np.full((C, C, C), F32(a[k]), F32) for k in range(3)]
                at[axis] = t
                for k in range(3):                                      # (an edge that does not cross adds +0, which changes no sum that started at +0)
                    total[k] = total[k] + np.where(crosses, at[k], F32(0))
                count += crosses
                g[axis] = g[axis] + (sb - sa)
        cz, cy, cx = np.nonzero(active)                                 # ascending (cz (N + 1) + cy) (N + 1) + cx
        n = count[active].astype(F32)
        pos = [total[k][active] / n + (c.astype(np.int32) - 1).astype(F32) for k, c in enumerate((cx, cy, cz))]
        gv = [g[k][active] for k in range(3)]
        len2 = gv[0] * gv[0] + gv[1] * gv[1] + gv[2] * gv[2]
        ok = np.isfinite(len2) & (len2 > 0)
        nrm = [np.where(ok, gv[k] / np.sqrt(len2), F32(0)).astype(F32) for k in range(3)]
        if space == SPACE_OBJECT:
            bound = np.asarray(bound, F32)
            q = [(pos[k] + F32(0.5)) / F32(N) * F32(2) - F32(1) for k in range(3)]
            q[1] = -q[1]
            nrm[1] = -nrm[1]
            pos = [q[k] * bound[3] + bound[k] for k in range(3)]
        vb = np.stack(pos + nrm, axis=1).astype(F32).reshape(-1, 6)

        # triangles: the edge from sample p along +axis belongs to the cell whose minimum corner is p
        number = np.full((C, C, C), -1, np.int64)
        number[active] = np.arange(len(cz))
        keys, quads = [], []
        for axis in range(3):
            u, w = (axis + 1) % 3, (axis + 2) % 3
            b = [0, 0, 0]
            b[axis] = 1
            first_in = corner((0, 0, 0), inside)
            crosses = first_in != corner(b, inside)
            oz, oy, ox = np.nonzero(crosses)
            owner = np.stack([ox, oy, oz], axis=1).astype(np.int64)     # = p + (1, 1, 1) = p + axis + u + w
            cells = []
            for du, dw in ((1, 1), (0, 1), (0, 0), (1, 0)):             # p + axis + {0, u, u + w, w}
                c = owner.copy()
                c[:, u] -= du
                c[:, w] -= dw
                assert (c >= 0).all()                                   # an edge in the outermost padding layer never crosses
                v = number[c[:, 2], c[:, 1], c[:, 0]]
                assert (v >= 0).all()
                cells.append(v)
            quad = np.stack(cells, axis=1)
            quad = np.where(first_in[oz, oy, ox][:, None], quad, quad[:, ::-1])
            keys.append(((oz * C + oy) * C + ox) * 3 + axis)
            quads.append(quad)
        keys, quads = np.concatenate(keys), np.concatenate(quads)
        quads = quads[np.argsort(keys, kind="stable")]
        tris = np.stack([quads[:, [0, 1, 2]], quads[:, [0, 2, 3]]], axis=1).reshape(-1, 3)
        if space == SPACE_OBJECT:
            tris = tris[:, ::-1]                                        # y is mirrored: (a, b, c) -> (c, b, a)
    return vb, np.ascontiguousarray(tris, np.int64).astype(np.uint32).reshape(-1)


# ---- what a closed, outward-oriented mesh is ---------------------------------------------------------------------------------------
def directed_edges_pair_up(ib):
    """every directed edge (a, b) occurs exactly as often as (b, a)"""
    t = np.asarray(ib, np.int64).reshape(-1, 3)
    e = np.concatenate([t[:, [0, 1]], t[:, [1, 2]], t[:, [2, 0]]])
    fwd, nf = np.unique(e[:, 0] << 32 | e[:, 1], return_counts=True)
    rev, nr = np.unique(e[:, 1] << 32 | e[:, 0], return_counts=True)
    return np.array_equal(fwd, rev) and np.array_equal(nf, nr)


def signed_volume(vb, ib):
    """sum over the triangles of a . (b x c) / 6 in float64: positive when (b - a) x (c - a) points out of the solid"""
    p = np.asarray(vb, np.float64)[:, :3]
    t = np.asarray(ib, np.int64).reshape(-1, 3)
    a, b, c = p[t[:, 0]], p[t[:, 1]], p[t[:, 2]]
    return float((a * np.cross(b, c)).sum() / 6.0)
