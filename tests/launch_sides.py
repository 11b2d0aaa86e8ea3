"""The sides, the mesh and the wanted results of the launch sweep (tests/test_launch_sides.py through the host-compiled code,
tests/test_gpu_launch_sides.py on the device).  The voxelizer's launch paths branch on residues of the side N and of a partition's height
nz -- N & 3 picks store_brick's byte stores or its dword row stores, N & 15 the clear inside the dispatch or the clear kernel in front
(whose byte count is then no multiple of 16), the brick counts' common power of two the Morton bits of the prepared queue, nz & 3 the rows
of a slab's last brick layer -- and the lanes of a brick that hangs over the grid's end repeat its last voxels and must store nothing.
So the sweep takes every even side up to 72 and three longer ones, with a mesh whose occupied AND empty voxels reach into all three last
brick layers: an overhanging lane that stores, a row store past nz, a clear that misses a ragged tail shows there as a wrong byte.

What makes a comparison with these results a test is asserted here, on the oracle alone, per side (Wanted): a device test that could
not fail is then a failed test.  A plain helper: no fixtures, no hooks."""
import numpy as np

SWEEP = list(range(2, 73, 2))            # every N % 16: 0 the clear in the dispatch, 4 / 8 / 12 dword rows behind the clear kernel, 2 mod 4 byte stores
WIDE = (100, 130, 194)                   # N % 16 = 4; N % 4 = 2 twice, above the automatic 128-texel map

assert {N % 16 for N in SWEEP} == set(range(0, 16, 2))
assert WIDE[0] % 16 == 4 and all(N % 4 == 2 and N > 128 for N in WIDE[1:])

_MESH, _WANT = [], {}


def mesh():
    """The sweep's mesh.  A shell: the six faces of the cube in patches on the lattice of a 4^3 grid, three in ten left out (holes: the parity
    rule's zeros), the normals random (the reference rule's zeros), one patch triangle in four there twice with other normals (an exact tie
    of t that only the texel image sees) -- the last brick layers of a grid see little else than the faces, so this is what fills them with
    both values.  And across two diagonals of the cube, at radius 1.5, 128 coincident copies of one small triangle: a ray that meets them
    descends both children at every level of their subtree, so a column of 8 entries runs out -- for the few rays along those diagonals,
    some of the 8 rays of a 2^3 grid among them, and for no other: 3 rays at 2^3, 35 at 34^3, 3,115 of 7.3 M at 194^3 on the device.  The
    redo pass takes 2^16 rays of a launch and the library refuses a forced column that more run out of (test_gpu_parity.py::
    test_errors_are_loud); a mesh of cube-spanning triangles -- lattice_mesh(default_rng(1011), 600, 4) meets every other condition --
    makes every ray run out, which the redo pass can be asked for up to 40^3 only."""
    if not _MESH:
        rng = np.random.default_rng(2)
        G, keep, twice, copies = 4, 0.7, 0.25, 128
        tris = []
        for axis in range(3):
            u, v = [a for a in range(3) if a != axis]
            for side in (-1.0, 1.0):
                for i in range(G):
                    for j in range(G):
                        if rng.random() > keep:
                            continue

                        def corner(a, b):
                            p = np.zeros(3)
                            p[axis], p[u], p[v] = side, -1 + 2 * a / G, -1 + 2 * b / G
                            return p
                        for t in ([corner(i, j), corner(i + 1, j), corner(i + 1, j + 1)], [corner(i, j), corner(i + 1, j + 1), corner(i, j + 1)]):
                            tris.append(t)
                            if rng.random() < twice:
                                tris.append(t)
        for d in ((1, 1, 1), (1, -1, 1)):
            d = np.array(d, float) / np.sqrt(3)
            a = np.cross(d, [0, 0, 1.0])
            a /= np.linalg.norm(a)
            b = np.cross(d, a)
            c, s = d * 1.5, 0.03
            tris += [[c + s * a, c - 0.5 * s * a + 0.87 * s * b, c - 0.5 * s * a - 0.87 * s * b]] * copies
        pos = np.asarray(tris, np.float64).reshape(-1, 3)
        pos = np.concatenate([pos, [[-1, -1, -1], [1, 1, 1]]]).astype(np.float32)      # pin the bound to the unit cube
        nrm = rng.normal(size=pos.shape).astype(np.float32)
        nrm /= np.linalg.norm(nrm, axis=1)[:, None]
        _MESH.append((np.concatenate([pos, nrm], axis=1).astype(np.float32), np.arange(3 * len(tris), dtype=np.uint32)))
    return _MESH[0]


def reversed_order(ib):
    """the same triangles, the last one first: another winner for every exact tie of t"""
    return np.ascontiguousarray(ib.reshape(-1, 3)[::-1].reshape(-1))


def overhang(N):
    """the first index of the last brick layer: the bricks from here on hang over the grid's end unless N is a multiple of 4"""
    return 4 * ((N - 1) // 4)


def border_layers(a):
    """the last brick layer of a [N, N, N] array in x, y and z"""
    lo = overhang(a.shape[0])
    return {"x": a[:, :, lo:], "y": a[:, lo:, :], "z": a[lo:]}


def border_shares(N, rule, g):
    """the solid share of each last brick layer of a wanted grid, asserted to lie in [0.10, 0.90] (N = 2: the grid holds both values)"""
    assert g.shape == (N, N, N) and set(np.unique(g)) == {0, 1}, (N, rule, g.shape, np.unique(g))
    shares = {axis: float(layer.mean()) for axis, layer in border_layers(g).items()} if N >= 4 else {}
    for axis, share in shares.items():
        assert 0.10 <= share <= 0.90, (N, rule, axis, share)
    return shares


class Wanted:
    """What the oracle says of mesh() at side N, each part computed when it is first asked for, its conditions asserted then, and never
    written to: ref = (grid, texel image) of the reference rule, parity = the parity rule's grid.  The conditions: in each last brick layer,
    under either rule, between a tenth and nine tenths of the voxels are solid; the image is non-zero exactly where the grid is and has zeros;
    and with the triangles in the opposite order the image differs in the last brick layer in z -- one of the three the contract names, and
    a slab of four slices at the most to compute -- so a tie that only the image sees is decided in an overhanging brick."""

    def __init__(self, orc, N, algo):
        self.orc, self.N, self.algo = orc, N, algo
        self.shares = {}
        self._ref = self._parity = None

    @property
    def ref(self):
        if self._ref is None:
            N = self.N
            vb, ib = mesh()
            grid, tex = self.orc.Scene(vb, ib).voxelize(N, algo=self.algo, texels=True)
            assert np.array_equal(tex != 0, grid != 0) and (tex == 0).any() and (tex != 0).any(), N
            self.shares["reference"] = border_shares(N, "reference", grid)
            lo = overhang(N)
            self.tied = self.orc.Scene(vb, reversed_order(ib)).voxelize(N, algo=self.algo, z0=lo, nz=N - lo, texels=True)[1]
            assert (self.tied != tex[lo:]).any(), (N, "no tie decides a texel of the last brick layer")
            for a in (grid, tex, self.tied):
                a.setflags(write=False)
            self._ref = (grid, tex)
        return self._ref

    @property
    def parity(self):
        if self._parity is None:
            vb, ib = mesh()
            g = self.orc.Scene(vb, ib).voxelize(self.N, mode=self.orc.MODE_PARITY, algo=self.algo)
            self.shares["parity"] = border_shares(self.N, "parity", g)
            g.setflags(write=False)
            self._parity = g
        return self._parity


def wanted(orc, N):
    """Wanted(N), one per side.  SWEEP sides: the oracle's brute force.  WIDE sides: its BVH, which tests/test_launch_sides.py shows equal
    to brute force, grid and image, both rules and both triangle orders, at every SWEEP side (brute force takes half a minute at 194^3)."""
    if N not in _WANT:
        _WANT[N] = Wanted(orc, N, orc.ALGO_BRUTE if N <= SWEEP[-1] else orc.ALGO_BVH)
    return _WANT[N]
