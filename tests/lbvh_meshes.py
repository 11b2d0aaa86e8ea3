"""Inputs of the LBVH build tests (tests/test_lbvh_rule.py, tests/test_gpu_lbvh.py): deterministic (name, vb, ib) triples, each
family aimed at one branch of csrc/lbvh.hip, the sort behind it or the header routines morton_key / karras_node / compress_node /
widen_node (DESIGN.md section 4.1 has the table of which case reaches which branch).

A family that needs a fixed bound pins it with two unreferenced vertices at (-1, -1, -1) and (1, 1, 1): centre 0, half width 1, so
the normalised position of a vertex is the vertex itself and a Morton cell q spans [q / 512 - 1, (q + 1) / 512 - 1) on its axis."""
import numpy as np

from dxrvoxelizer_amd import meshes

COUNTS = (1, 2, 3, 4, 5, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 2047, 2048, 2049, 4095, 4097, 65535, 65536, 65537, 65793, 131073)
COPIES = (2, 1024, 1025, 4097)
COMB_BITS = (7, 8, 12, 16)
FUSED_BOUNDARY = (2097152, 2097153)          # the last count of the fused gather + hierarchy launch (and of the small sort), and the first beyond
RUN_LENGTHS = (1, 2, 3, 64, 257)


def _with_normals(pos, pin):
    """(T, 3, 3) float32 positions -> (vb, ib): three private vertices per triangle, face normals in float32, then the two pins"""
    pos = np.ascontiguousarray(pos, np.float32)
    T = len(pos)
    a, b = pos[:, 1] - pos[:, 0], pos[:, 2] - pos[:, 1]
    n = np.cross(a.astype(np.float64), b.astype(np.float64))
    ln = np.sqrt((n * n).sum(1))
    n[ln == 0] = (0.0, 0.0, 1.0)                             # (no family makes one on purpose; a normal is never NaN here)
    ln[ln == 0] = 1.0
    n = (n / ln[:, None]).astype(np.float32)
    vb = np.empty((3 * T + (2 if pin else 0), 6), np.float32)
    vb[:3 * T, :3] = pos.reshape(-1, 3)
    vb[:3 * T, 3:] = np.repeat(n, 3, axis=0)
    if pin:
        vb[3 * T] = (-1, -1, -1, 0, 0, 1)
        vb[3 * T + 1] = (1, 1, 1, 0, 0, 1)
    return vb, np.arange(3 * T, dtype=np.uint32)


def pinned(vb, ib, r=1.0):
    """the same mesh with two pins at -+(r, r, r) behind its vertices (which must lie inside [-r, r]^3): centre 0, half width r"""
    assert float(np.abs(vb[:, :3]).max()) <= r
    pins = np.array([[-r, -r, -r, 0, 0, 1], [r, r, r, 0, 0, 1]], np.float32)
    return np.vstack([vb, pins]), ib


def count(T):
    vb, ib = meshes.soup(T, seed=77 + T, edge=0.2)
    return f"count-{T}", vb, ib


def copies(T):
    """one triangle T times: a single run of equal Morton codes, the index half of the key decides everything"""
    vb = np.zeros((5, 6), np.float32)
    vb[:3, :3] = [[-0.9, -0.9, 0.4], [0.9, -0.9, 0.4], [0.0, 0.9, 0.4]]
    vb[:3, 3:] = [0.57735, 0.57735, 0.57735]
    vb[3, :3], vb[4, :3] = [-1, -1, -1], [1, 1, 1]
    return f"copies-{T}", vb, np.tile(np.arange(3, dtype=np.uint32), T)


def cell_centre(q):
    return (np.asarray(q, np.float64) + 0.5) / 512.0 - 1.0


def code_cell(code):
    """(qx, qy, qz) of a 30-bit Morton code: z in the lowest bit of each triple, then y, then x (morton_key)"""
    q = [0, 0, 0]
    for bit in range(10):
        q[2] |= ((code >> (3 * bit)) & 1) << bit
        q[1] |= ((code >> (3 * bit + 1)) & 1) << bit
        q[0] |= ((code >> (3 * bit + 2)) & 1) << bit
    return q


def _small_tris(rng, centres, edge):
    """a triangle around every centre whose box centre stays within edge of it"""
    T = len(centres)
    off = rng.uniform(-edge / 2, edge / 2, (T, 3, 3))
    off -= (off.max(1, keepdims=True) + off.min(1, keepdims=True)) / 2        # box centre on the cell centre (up to rounding)
    return (np.asarray(centres, np.float64)[:, None, :] + off).astype(np.float32)


def runs():
    """about 3 000 triangles in a few hundred Morton cells: runs of 1, 2, 3, 64 and 257 equal codes next to each other and to single
    keys, the triangles of a run scattered over the index range"""
    rng = np.random.default_rng(4242)
    lengths = np.array([257] * 4 + [64] * 14 + [3] * 150 + [2] * 150 + [1] * 130)
    rng.shuffle(lengths)
    cells = set()
    while len(cells) < len(lengths):                                          # clusters of neighbouring cells: equal high bits, distinct low ones
        base = rng.integers(0, 1016, 3)
        for _ in range(4):
            cells.add(tuple(int(v) for v in base + rng.integers(0, 8, 3)))
    cells = np.array(sorted(cells))[:len(lengths)]
    q = np.repeat(cells, lengths, axis=0)
    q = q[rng.permutation(len(q))]
    vb, ib = _with_normals(_small_tris(rng, cell_centre(q), 2.0 ** -12), pin=True)
    return "runs", vb, ib


def comb(b):
    """T = 2^b + 1 triangles, height 31 + b: the 31 codes `top k bits one, the rest zero` (k = 0 .. 30) make a chain of 30 levels, the
    cell of k = 30 holds the 2 + b triangles 0, 1, 2, 4, ..., 2^b whose index bits make a chain of b + 1 more; every other triangle lies
    in the low octant (all three top bits zero)."""
    rng = np.random.default_rng(900 + b)
    T = (1 << b) + 1
    q = rng.integers(0, 512, (T, 3))
    chain = [0] + [1 << e for e in range(b + 1)]
    free = [i for i in range(T) if i not in set(chain)]
    full = (1 << 30) - 1
    for i in chain:
        q[i] = code_cell(full)
    for k in range(30):
        q[free[k]] = code_cell(full ^ ((1 << (30 - k)) - 1))
    vb, ib = _with_normals(_small_tris(rng, cell_centre(q), 2.0 ** -12), pin=True)
    return f"comb-{b}", vb, ib


def comb_soup():
    """comb-8 with a dense soup of large triangles behind it: as high as the comb (a key more never lowers a radix tree), and rays that
    cross many sibling boxes -- the combs' own triangles are so small that no ray ever holds more than a few entries, however high
    the tree"""
    _, vb, ib = comb(8)
    T = len(ib) // 3
    svb, _ = meshes.soup(3000, seed=812, extent=0.6, edge=0.3)
    pos = np.concatenate([vb[:3 * T, :3].reshape(-1, 3, 3), svb[:, :3].reshape(-1, 3, 3)])
    vb, ib = _with_normals(pos, pin=True)
    return "comb-8-soup", vb, ib


def flat(axis):
    """a soup of 3 000 with one coordinate constant: the box is two pads thick there and every key has one coordinate in common"""
    vb, ib = meshes.soup(3000, seed=31 + axis, edge=0.2)
    pos = vb[:, :3].reshape(-1, 3, 3).copy()
    pos[:, :, axis] = np.float32(0.25)
    vb, ib = _with_normals(pos, pin=False)
    return f"flat-{'xyz'[axis]}", vb, ib


def clamped():
    """a soup inside the pinned bound plus triangles that lie in the bound's faces and at its corners: centres at -1 (quant10's lower
    clamp, u = 0) and at or next to +1 (u >= 1024, the upper clamp)"""
    vb, ib = meshes.soup(1500, seed=58, extent=0.7, edge=0.2)
    pos = [vb[:, :3].reshape(-1, 3, 3)]
    e = 2.0 ** -12
    rng = np.random.default_rng(59)
    for axis in range(3):
        for side in (-1.0, 1.0):
            for _ in range(6):                                                # in the face: the axis coordinate is side itself
                c = rng.uniform(-0.9, 0.9, 3)
                t = c[None, :] + rng.uniform(-0.05, 0.05, (3, 3))
                t[:, axis] = side
                pos.append(t[None].astype(np.float32))
    for sx in (-1.0, 1.0):
        for sy in (-1.0, 1.0):
            for sz in (-1.0, 1.0):                                            # at the corner, in the face x = sx
                s = np.array([sx, sy, sz])
                t = np.array([s, s - [0, 0, sz * e], s - [0, sy * e, 0]])
                pos.append(t[None].astype(np.float32))
    vb, ib = _with_normals(np.concatenate(pos), pin=True)
    return "clamped", vb, ib


def giant_and_tiny():
    """2 000 triangles whose boxes are the pad and a few ulps, and three that span the bound"""
    rng = np.random.default_rng(61)
    tiny = (rng.uniform(-0.9, 0.9, (2000, 1, 3)) + rng.uniform(-2e-7, 2e-7, (2000, 3, 3))).astype(np.float32)
    big = np.array([[[-1, -1, -1], [1, -1, 0.5], [0, 1, 1]],
                    [[-1, 1, -0.99], [1, 1, -1], [0.25, -1, 1]],
                    [[1, -1, 1], [-1, 0.99, 1], [-0.5, 1, -1]]], np.float32)
    pos = np.concatenate([tiny[:1000], big, tiny[1000:]])
    vb, ib = _with_normals(pos, pin=True)
    return "giant-and-tiny", vb, ib


def fused_boundary(T):
    vb, ib = meshes.soup(T, seed=9, edge=0.02)
    return f"fused-{T}", vb, ib


_MAKERS = {}
for _T in COUNTS:
    _MAKERS[f"count-{_T}"] = (count, _T)
for _T in COPIES:
    _MAKERS[f"copies-{_T}"] = (copies, _T)
_MAKERS["runs"] = (runs,)
for _b in COMB_BITS:
    _MAKERS[f"comb-{_b}"] = (comb, _b)
_MAKERS["comb-8-soup"] = (comb_soup,)
for _a in range(3):
    _MAKERS[f"flat-{'xyz'[_a]}"] = (flat, _a)
_MAKERS["clamped"] = (clamped,)
_MAKERS["giant-and-tiny"] = (giant_and_tiny,)

NAMES = tuple(_MAKERS)                       # every case but the two of the fused launch's boundary
_CACHE = {}


def get(name):
    """(vb, ib) of a named case; made once per process, never written to"""
    if name not in _CACHE:
        fn, *args = _MAKERS[name]
        _, vb, ib = fn(*args)
        vb.setflags(write=False)
        ib.setflags(write=False)
        _CACHE[name] = (vb, ib)
    return _CACHE[name]


def moved(vb, ib, seed, amount=0.01):
    """every referenced vertex moved by up to `amount` per coordinate and clipped into the bound the unreferenced pins span; the pins
    stay, so the bound does"""
    rng = np.random.default_rng(seed)
    out = np.array(vb, np.float32)
    used = np.unique(ib)
    r = float(np.abs(vb[:, :3]).max())
    out[used, :3] += rng.uniform(-amount, amount, (len(used), 3)).astype(np.float32)
    out[used, :3] = np.clip(out[used, :3], -r, r)
    return out
