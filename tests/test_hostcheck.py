"""Host logic of the PRODUCT: its __host__ __device__ arithmetic, Karras hierarchy rule and
traversal (dxrvoxelizer_amd/csrc/dxv_math.h, dxv_trace.h) compiled for the CPU by
tests/hostcheck and compared bit for bit with the oracle.  The GPU kernels instantiate exactly
this code; the -m gpu tests then only have to prove the device build, sort and launch."""
import numpy as np
import pytest

from dxrvoxelizer_amd import meshes


def check_tree(nodes, T):
    """Every leaf and every internal node reachable exactly once; child boxes finite; heights."""
    c = nodes[:, 12:14].view(np.int32)
    seen_leaf = np.zeros(T, np.int32)
    seen_node = np.zeros(max(T - 1, 1), np.int32)
    stack = [0]
    while stack:
        n = stack.pop()
        seen_node[n] += 1
        for link in c[n]:
            if link < 0:
                seen_leaf[~link] += 1
            else:
                stack.append(int(link))
    assert np.all(seen_leaf == 1) and np.all(seen_node == 1)
    boxes = nodes[:, :12].view(np.float32)
    assert np.isfinite(boxes).all()
    assert np.all(boxes[:, 0:3] <= boxes[:, 3:6]) and np.all(boxes[:, 6:9] <= boxes[:, 9:12])


@pytest.mark.parametrize("name", ["bunny", "dragon", "turingbowl"])
def test_host_lbvh_equals_oracle_assets(orc, hostcheck, request, name):
    vb, ib, _ = request.getfixturevalue(name)
    s = orc.Scene(vb, ib)
    h = hostcheck(vb, ib, s.bound)
    check_tree(h.nodes(), h.T)
    keys = h.keys()
    assert np.all(keys[1:] > keys[:-1])
    assert 1 <= h.height <= 62
    # 2/3 = postponed-leaf walks, 5 (-> 4) = parity rows, 6 = postponed-leaf walk over the wide nodes
    for N, mode in ((32, 0), (32, 1), (64, 0), (64, 2), (64, 3), (64, 5), (64, 6), (64, 7), (30, 9), (64, 11), (30, 13)):   # 7, 9 (-> 8): row blocks; 11, 13 (-> 10): four-box walk
        g, ovf = h.voxelize(N, {5: 4, 9: 8, 13: 10}.get(mode, mode), stack=h.height + 3 if mode != 6 else 3 * ((h.height + 1) // 2) + 5)
        assert not ovf
        assert np.array_equal(g, s.voxelize(N, mode=mode % 2))


def test_host_texels_equal_oracle(orc, hostcheck, bunny):
    vb, ib, _ = bunny
    s = orc.Scene(vb, ib)
    h = hostcheck(vb, ib, s.bound)
    g, tex, ovf = h.voxelize(32, 0, texels=True)
    og, otex = s.voxelize(32, texels=True)
    assert not ovf and np.array_equal(g, og) and np.array_equal(tex, otex)


@pytest.mark.parametrize("gen,args", [("cube", ()), ("tetrahedron", ()), ("uv_sphere", (24, 12)), ("torus", (60, 30)),
                                      ("soup", (3000,))])
def test_host_lbvh_equals_oracle_brute_synthetic(orc, hostcheck, gen, args):
    vb, ib = getattr(meshes, gen)(*args)
    s = orc.Scene(vb, ib)
    h = hostcheck(vb, ib, s.bound)
    check_tree(h.nodes(), h.T)
    modes = (0, 2, 6) if gen == "soup" else (0, 1, 2, 3, 5, 6)
    for mode in modes:
        g, ovf = h.voxelize(16, 4 if mode == 5 else mode)
        assert not ovf
        assert np.array_equal(g, s.voxelize(16, mode=mode % 2, algo=orc.ALGO_BRUTE))


def test_single_triangle_and_duplicates(orc, hostcheck):
    """T == 1 (dummy sibling) and many identical triangles (equal Morton codes -> index bits
    decide the hierarchy)."""
    vb = np.zeros((5, 6), np.float32)
    vb[:3, :3] = [[-0.9, -0.9, 0.4], [0.9, -0.9, 0.4], [0.0, 0.9, 0.4]]
    vb[:3, 3:] = [0.57735, 0.57735, 0.57735]
    vb[3, :3], vb[4, :3] = [-1, -1, -1], [1, 1, 1]
    one = np.arange(3, dtype=np.uint32)
    s = orc.Scene(vb, one)
    h = hostcheck(vb, one, s.bound)
    for mode in (0, 1, 2, 3):
        g, ovf = h.voxelize(16, mode)
        assert not ovf and np.array_equal(g, s.voxelize(16, mode=mode % 2, algo=orc.ALGO_BRUTE))
    many = np.tile(one, 37)
    s = orc.Scene(vb, many)
    h = hostcheck(vb, many, s.bound)
    check_tree(h.nodes(), h.T)
    for mode in (0, 2):
        g, ovf = h.voxelize(16, mode)
        assert not ovf and np.array_equal(g, s.voxelize(16, algo=orc.ALGO_BRUTE))
    for mode in (1, 3):
        g, ovf = h.voxelize(16, mode)
        assert np.array_equal(g, s.voxelize(16, mode=1, algo=orc.ALGO_BRUTE))


def test_stack_overflow_is_reported(orc, hostcheck, bunny):
    vb, ib, _ = bunny
    s = orc.Scene(vb, ib)
    h = hostcheck(vb, ib, s.bound)
    for mode in (0, 2):
        _, ovf = h.voxelize(32, mode, stack=2 if mode == 0 else 5)
        assert ovf


def test_slab_concatenation_equals_full_grid(orc, hostcheck, dragon):
    vb, ib, _ = dragon
    s = orc.Scene(vb, ib)
    h = hostcheck(vb, ib, s.bound)
    from dxrvoxelizer_amd.slabs import gather_slabs, slab_range
    full, _ = h.voxelize(32, 0)
    parts = []
    for r in range(8):
        z0, nz = slab_range(32, r, 8)
        parts.append((z0, h.voxelize(32, 0, z0=z0, nz=nz)[0]))
    assert np.array_equal(gather_slabs(parts), full)


def test_half_conversions_are_outward_and_tight(hostcheck):
    """Traversal nodes store half-float boxes rounded outward (dxv_math.h half_down / half_up): the
    stored box must contain the exact one and be the tightest representable."""
    L = hostcheck.lib
    rng = np.random.default_rng(3)
    xs = np.concatenate([rng.uniform(-1.1, 1.1, 20000), rng.normal(0, 1e-3, 5000), [0.0, -0.0, 1.0, -1.0, 65504.0, 1e30, -1e30, 1e-9]])
    for x in xs.astype(np.float32):
        d, u = L.hc_half_down(x), L.hc_half_up(x)
        fd, fu = L.hc_half_to_float(d), L.hc_half_to_float(u)
        assert fd <= x <= fu
        hd, hu = np.float16(fd), np.float16(fu)                    # numpy: exact f16 values
        if abs(x) < 60000:
            assert np.nextafter(hd, np.float16(np.inf)) > x or float(hd) == float(x)
            assert np.nextafter(hu, np.float16(-np.inf)) < x or float(hu) == float(x)


def test_compressed_nodes_contain_exact_boxes(orc, hostcheck, dragon):
    vb, ib, _ = dragon
    s = orc.Scene(vb, ib)
    h = hostcheck(vb, ib, s.bound)
    exact = h.nodes()[:, :12].view(np.float32)
    packed = h.nodes32()
    halves = packed[:, :6].copy().view(np.uint16).view(np.float16).astype(np.float32).reshape(-1, 12)
    # Node32 is axis-major {lo0 lo1 hi0 hi1} x 3; the exact node is child-major lo.xyz hi.xyz x 2
    halves = halves.reshape(-1, 3, 2, 2).transpose(0, 3, 2, 1).reshape(-1, 12)
    assert np.array_equal(packed[:, 6:8], h.nodes()[:, 12:14])     # links unchanged
    for c in (0, 6):
        assert np.all(halves[:, c:c + 3] <= exact[:, c:c + 3]) and np.all(halves[:, c + 3:c + 6] >= exact[:, c + 3:c + 6])
    assert np.max(np.abs(halves - exact)) < 1e-3                   # half ulp near 1.0 is 2^-11


def test_wide_nodes_hold_the_grandchildren(orc, hostcheck, dragon):
    """Node64 of binary node i: every internal child replaced by its two children, boxes rounded
    outward, unused slots inverted (never hit) -- and the same packing of the exact boxes as Node32."""
    vb, ib, _ = dragon
    s = orc.Scene(vb, ib)
    h = hostcheck(vb, ib, s.bound)
    nodes = h.nodes()
    exact = nodes[:, :12].view(np.float32).reshape(-1, 2, 2, 3)     # [node][child][lo/hi][axis]
    links = nodes[:, 12:14].view(np.int32)
    wide = h.nodes64()
    planes = wide[:, :12].copy().view(np.uint16).view(np.float16).astype(np.float32).reshape(-1, 3, 2, 4)   # [axis][side][slot]
    wl = wide[:, 12:16].view(np.int32)
    rng = np.random.default_rng(5)
    for i in rng.integers(0, len(nodes), 400):
        want = []
        for side in range(2):
            c = links[i, side]
            if c >= 0:
                want += [(exact[c, 0], links[c, 0]), (exact[c, 1], links[c, 1])]
            else:
                want.append((exact[i, side], c))
        for slot in range(4):
            lo, hi = planes[i, :, 0, slot], planes[i, :, 1, slot]
            if slot < len(want):
                box, link = want[slot]
                assert wl[i, slot] == link
                assert np.all(lo <= box[0]) and np.all(hi >= box[1]) and np.max(np.abs(lo - box[0])) < 1e-3
            else:
                assert wl[i, slot] == -2 ** 31 and np.all(np.isposinf(lo)) and np.all(np.isneginf(hi))


def test_queued_walk_every_capacity_is_exact_or_reports_overflow(orc, hostcheck, dragon):
    """The stack and the postponed-leaf queue share one LDS column.  For every column size the walk
    must either report overflow or produce the exact grid -- never a silently wrong one (a lane whose
    stack alone no longer leaves room after a flush has to stop)."""
    vb, ib, _ = dragon
    s = orc.Scene(vb, ib)
    h = hostcheck(vb, ib, s.bound)
    want = {0: s.voxelize(32), 1: s.voxelize(32, mode=1)}
    clean = 0
    for cap in range(5, 26):
        for mode in (2, 3, 6):
            g, ovf = h.voxelize(32, mode, stack=cap)
            if not ovf:
                clean += 1
                assert np.array_equal(g, want[mode % 2]), (cap, mode)
            else:                                   # rays that did not overflow are still right
                bad = g != want[mode % 2]
                assert bad.mean() < 0.2, (cap, mode)
    assert clean >= 15


def test_direction_space_lists_give_the_tree_walk_grid(orc, hostcheck, bunny):
    """The reference rule through the direction-space lists (dxv_dirmap.h: footprints, list order, the
    two-step scan with a small queue) equals the tree walk and the oracle's brute force -- on the
    bunny, on lattice-snapped adversarial triangles (shared edges and vertices, degenerate and
    coplanar duplicates, triangles through the grid centre) and for coarse and fine maps."""
    from test_fuzz import lattice_mesh
    vb, ib, _ = bunny
    s = orc.Scene(vb, ib)
    h = hostcheck(vb, ib, s.bound)
    want, _ = h.voxelize(64, mode=0)
    for R in (32, 256):
        cells, entries = h.lists(R)
        begin, count, r1max = cells[:, 0].astype(np.int64), (cells[:, 1] & 0xffff).astype(np.int64), cells[:, 1] >> 16
        full = count > 0
        assert int((begin + count).max()) == len(entries) and int(count.sum()) == len(entries)
        assert np.array_equal(r1max[full], (entries[(begin + count)[full] - 1, 2] >> 16) & 0x7fff)   # far radius of the last entry
        assert (entries[:, 2] & 0x80008000 == 0x80008000).all() and (entries[:, 0] & 0x80808080 == 0).all()
        r1 = ((entries[:, 2] >> 16) & 0x7fff).astype(np.int64)
        for k in np.flatnonzero(full)[:: max(1, int(full.sum()) // 50)]:                           # lists are sorted by far radius
            assert (np.diff(r1[begin[k]:begin[k] + count[k]]) >= 0).all()
        k = int(np.argmax(count))                                                                  # the search hints of the longest list
        if count[k] > 8:
            assert (cells[k, 3] & 0xffff) == r1[begin[k] + count[k] // 2]
        assert (entries[:, 1] != 0).mean() > 0.2                                                   # a good part of the entries carries an edge
        got, ovf = h.voxelize(64, mode=12, stack=4)                   # a queue of four entries: several flushes per ray
        assert ovf == 0 and np.array_equal(got, want), R
    rng = np.random.default_rng(99)
    for n_tris in (1, 2, 3, 7, 30, 200):
        for N in (8, 16, 32):
            vb, ib = lattice_mesh(rng, n_tris, N)
            s = orc.Scene(vb, ib)
            h = hostcheck(vb, ib, s.bound)
            want = s.voxelize(N, algo=orc.ALGO_BRUTE)
            for R in (16, 128):
                h.lists(R)
                got, ovf = h.voxelize(N, mode=12, stack=8)
                assert ovf == 0 and np.array_equal(got, want), (n_tris, N, R)


def test_ray_side_half_conversions_equal_the_general_ones(hostcheck):
    """dm_half_down_pos / dm_half_up_pos (two integer instructions, what a ray uses for its radii in the lists' integer
    radial test) == half_down / half_up on their domain: positive floats in the half's normal range [2^-14, 65504)."""
    L = hostcheck.lib
    rng = np.random.default_rng(7)
    xs = np.concatenate([
        np.float32(2.0) ** rng.uniform(-14, 15.99, 20000).astype(np.float32),
        np.array([2.0 ** -14, 0.999, 1.0, 1.0009765625, 1.001, 1.73, 1.75, 4e-4, 65503.9, 10010.0], np.float32),
        (np.arange(1, 0x7bff, 7, dtype=np.uint32).astype(np.uint16).view(np.float16)).astype(np.float32)[15:],   # exact halfs (normal ones)
    ]).astype(np.float32)
    xs = xs[(xs >= np.float32(2.0 ** -14)) & (xs < np.float32(65504.0))]
    for x in xs[:: max(1, len(xs) // 6000)]:
        assert L.hc_dm_half_pos(float(x), 0) == L.hc_half_down(float(x)), x
        assert L.hc_dm_half_pos(float(x), 1) == L.hc_half_up(float(x)), x


def _dm_point(p):
    """face, u, v, radius of point p in direction space (dm_ray_point, dxv_dirmap.h)"""
    a = np.abs(p)
    ax = 0 if (a[0] >= a[1] and a[0] >= a[2]) else (1 if a[1] >= a[2] else 2)
    b, c = (ax + 1) % 3, (ax + 2) % 3
    return 2 * ax + (1 if p[ax] < 0 else 0), p[b] / a[ax], p[c] / a[ax], float(np.linalg.norm(p))


def test_footprints_contain_every_point_of_the_triangle(hostcheck):
    """dm_footprint's rectangle and radial range (builder side of the lists) against dense samples of the triangle itself:
    every sampled point lies inside the footprint of the face that sees it.  Lattice-snapped triangles put vertices and
    edges exactly on frustum corners and side planes, where the clip leaves coincident vertices behind (the soak of round 2
    found a near radius 3 % too large there: the perpendicular foot was judged outside its own polygon by rounding noise)."""
    import ctypes as C
    L = hostcheck.lib
    f32p = np.ctypeslib.ndpointer(np.float32, flags="C")
    L.hc_dm_footprint.argtypes = [f32p, C.c_uint32, f32p]
    rng = np.random.default_rng(4242)
    w = np.linspace(0.0, 1.0, 25)
    b1, b2 = np.meshgrid(w, w)
    keep = b1 + b2 <= 1.0
    b1, b2 = b1[keep], b2[keep]
    tris = [np.array([[0.25, -0.3125, -0.3125], [0.1875, -0.625, 0.8125], [0.875, 1.0, 1.0]], np.float32)]   # the soak's triangle
    for N in (4, 8, 16, 32):
        tris += list(rng.integers(-N, N + 1, size=(150, 3, 3)).astype(np.float32) / np.float32(N))
    tris += list(rng.uniform(-1, 1, size=(150, 3, 3)).astype(np.float32))
    out = np.zeros(6, np.float32)
    checked = 0
    for t in tris:
        fp = {}
        for f in range(6):
            if L.hc_dm_footprint(np.ascontiguousarray(t.reshape(-1)), f, out):
                fp[f] = out.copy()
        pts = t[0][None, :].astype(np.float64) * (1 - b1 - b2)[:, None] + t[1][None, :] * b1[:, None] + t[2][None, :] * b2[:, None]
        for p in pts:
            if np.abs(p).max() < 1e-3:
                continue
            f, u, v, rad = _dm_point(p)
            assert f in fp, (t, p)
            u0, u1, v0, v1, r0, r1 = fp[f]
            assert u0 <= u <= u1 and v0 <= v <= v1 and r0 <= rad <= r1, (t.tolist(), p.tolist(), f, fp[f].tolist(), (u, v, rad))
            checked += 1
    assert checked > 150000


def test_radial_range_per_texel_holds_every_point_of_the_triangle_there(hostcheck):
    """dm_local_radial (dxv_dirmap.h): the radial range of an entry cut to its texel.  Points of the triangle whose direction
    falls into texel (i, j) of a face must have their radius inside that texel's range -- for big, small, steep, nearly
    edge-on and near-centre triangles, on coarse and fine maps; and the cut must be worth something (on big footprints the
    mean range shrinks a lot)."""
    import ctypes as C
    L = hostcheck.lib
    f32p = np.ctypeslib.ndpointer(np.float32, flags="C")
    L.hc_dm_local_radial.argtypes = [f32p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, f32p]
    L.hc_dm_texel_outside.argtypes = [f32p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32]
    rng = np.random.default_rng(515)
    tris = list(rng.uniform(-1, 1, size=(120, 3, 3)).astype(np.float32))                       # big
    c = rng.uniform(-0.9, 0.9, size=(120, 1, 3))
    tris += list((c + rng.uniform(-0.15, 0.15, size=(120, 3, 3))).astype(np.float32))         # a few texels
    d = rng.normal(size=(60, 3)); d /= np.linalg.norm(d, axis=1)[:, None]
    for k in range(60):                                                                        # nearly edge-on: two vertices almost on one ray
        a = d[k] * rng.uniform(0.2, 0.5); b = d[k] * rng.uniform(0.6, 0.95) + rng.normal(size=3) * 1e-3
        tris.append(np.array([a, b, a + rng.normal(size=3) * 0.2], np.float32))
    tris += list((rng.uniform(-1, 1, size=(40, 3, 3)) * np.array([1, 1, 0.02])).astype(np.float32))   # planes near the centre
    w = rng.uniform(0, 1, size=(4000, 2))
    w = w[w.sum(1) <= 1.0]
    out = np.zeros(4, np.float32)
    checked = cut = 0
    whole = local = 0.0
    for R in (32, 256):
        for t in tris:
            pts = t[0].astype(np.float64) * (1 - w.sum(1))[:, None] + t[1].astype(np.float64) * w[:, :1] + t[2].astype(np.float64) * w[:, 1:]
            pts = pts[np.abs(pts).max(1) > 1e-2]
            a = np.abs(pts).argmax(1)
            ax = pts[np.arange(len(pts)), a]
            face = 2 * a + (ax < 0)
            u = pts[np.arange(len(pts)), (a + 1) % 3] / np.abs(ax)
            v = pts[np.arange(len(pts)), (a + 2) % 3] / np.abs(ax)
            rad = np.linalg.norm(pts, axis=1)
            ti = np.clip(((u + 1) * 0.5 * R).astype(int), 0, R - 1)
            tj = np.clip(((v + 1) * 0.5 * R).astype(int), 0, R - 1)
            # (points within 1e-6 of a texel border may belong to the neighbour: the builder and the kernel use float arithmetic)
            fu, fv = (u + 1) * 0.5 * R - ti, (v + 1) * 0.5 * R - tj
            inner = (fu > 1e-3) & (fu < 1 - 1e-3) & (fv > 1e-3) & (fv < 1 - 1e-3)
            cells = {}
            for k in np.nonzero(inner)[0][:600]:
                cells.setdefault((int(face[k]), int(ti[k]), int(tj[k])), []).append(rad[k])
            for (f, i, j), rs in cells.items():
                kind = L.hc_dm_local_radial(np.ascontiguousarray(t.reshape(-1)), f, R, i, j, out)
                assert kind != 0, (t.tolist(), f, i, j)
                # ... and a texel that holds a point of the triangle keeps its entry (dm_texel_outside)
                assert L.hc_dm_texel_outside(np.ascontiguousarray(t.reshape(-1)), f, R, i, j) == 0, (t.tolist(), R, f, i, j)
                g0, g1, l0, l1 = (float(x) for x in out)
                assert g0 <= l0 <= l1 <= g1
                assert l0 <= min(rs) and max(rs) <= l1, (t.tolist(), R, f, i, j, (g0, g1), (l0, l1), (min(rs), max(rs)))
                checked += len(rs)
                if kind == 2:
                    cut += 1; whole += g1 - g0; local += l1 - l0
    assert checked > 100000 and cut > 5000
    assert local < 0.5 * whole, (local, whole)           # over footprints of many texels the ranges shrink by more than half on average


def frustum_corner_case():
    """Known-answer case of the round-2 soak failure (seed 77001): a triangle whose edge runs through a frustum corner, hit
    by the ray of voxel (63, 54, 45) at 96^3 at radius 0.3692, next to the foot of the perpendicular from the grid centre
    (0.3676; the builder said 0.3777), and a small triangle across the same ray at radius 0.373 with the opposite normal:
    the first is the closest hit (voxel set); dropping it as "starts beyond the hit" leaves the second (voxel clear)."""
    tri = np.array([[0.25, -0.3125, -0.3125], [0.1875, -0.625, 0.8125], [0.875, 1.0, 1.0]], np.float64)
    o = np.array([(63 + 0.5) / 96 * 2 - 1, -((54 + 0.5) / 96 * 2 - 1), (45 + 0.5) / 96 * 2 - 1])
    d = o / np.linalg.norm(o)
    a = np.cross(d, [0.0, 0.0, 1.0]); a /= np.linalg.norm(a)
    b = np.cross(d, a)
    c = d * 0.373
    small = np.array([c + 0.01 * a, c - 0.005 * a + 0.009 * b, c - 0.005 * a - 0.009 * b])
    pos = np.concatenate([small, tri, [[-1, -1, -1], [1, 1, 1]]]).astype(np.float32)
    nrm = np.concatenate([np.tile(-d, (3, 1)), np.tile(d, (5, 1))]).astype(np.float32)
    return np.concatenate([pos, nrm], axis=1).astype(np.float32), np.arange(6, dtype=np.uint32)


def test_list_near_radius_through_a_frustum_corner(orc, hostcheck):
    vb, ib = frustum_corner_case()
    s = orc.Scene(vb, ib)
    want = s.voxelize(96, algo=orc.ALGO_BRUTE)
    assert want[45, 54, 63] == 1 and s.voxel(96, 63, 54, 45, algo=orc.ALGO_BRUTE)[2] == 1
    h = hostcheck(vb, ib, s.bound)
    for R in (16, 64, 256):
        h.lists(R)
        got, ovf = h.voxelize(96, mode=12, stack=8)
        assert ovf == 0 and np.array_equal(got, want), R


def test_normal_class_agrees_with_the_predicate_everywhere_on_the_triangle(hostcheck, bunny, dragon):
    """normal_class (dxv_math.h) classifies a triangle once for all rays that can hit it.  Every ray of the reference rule is
    radial, so the predicate at a hit point is  cos(angle(N(b), p(b))) > 0.12  with the interpolated normal and position:
    sampled densely over classified triangles it must always give the class, and by far more than rounding (the classes keep
    2e-3 rad of margin).  Triangles: smooth-ish fields around the threshold angle, random ones, degenerate normals, vertices
    near the grid centre; and the assets, where most triangles must be classified for the shortcut to be worth anything."""
    import ctypes as C
    L = hostcheck.lib
    f32p = np.ctypeslib.ndpointer(np.float32, flags="C")
    L.hc_normal_class.argtypes = [f32p, f32p]
    L.hc_normal_class.restype = C.c_uint32
    rng = np.random.default_rng(31337)
    w = np.linspace(-1e-6, 1.0 + 1e-6, 21)                     # a hair beyond the edges, like the hit test's barycentrics
    b1, b2 = np.meshgrid(w, w)
    keep = b1 + b2 <= 1.0 + 2e-6
    b1, b2 = b1[keep][:, None], b2[keep][:, None]
    thr = np.arccos(0.12)
    counts = {0: 0, 2: 0, 3: 0}
    closest = np.inf
    for it in range(6000):
        c = rng.normal(size=3); c *= rng.uniform(0.02, 1.7) / np.linalg.norm(c)
        size = 10.0 ** rng.uniform(-3, -0.3)
        tri = (c + rng.normal(size=(3, 3)) * size).astype(np.float32)
        # a normal at a chosen angle from the radial direction, often near the threshold; then perturbed per vertex
        d = c / np.linalg.norm(c)
        t = np.cross(d, rng.normal(size=3)); t /= np.linalg.norm(t)
        ang = thr + rng.normal() * 0.15 if it % 2 else rng.uniform(0, np.pi)
        n = np.cos(ang) * d + np.sin(ang) * t
        nrm = (n + rng.normal(size=(3, 3)) * 10.0 ** rng.uniform(-3, -0.2)) * rng.uniform(0.3, 3.0, size=(3, 1))
        if it % 97 == 0:
            nrm[rng.integers(0, 3)] = 0.0                      # a zero normal: never classified
        nrm = nrm.astype(np.float32)
        cls = L.hc_normal_class(np.ascontiguousarray(tri.reshape(-1)), np.ascontiguousarray(nrm.reshape(-1)))
        counts[cls] += 1
        if it % 97 == 0:
            assert cls == 0
        if cls == 0:
            continue
        P = tri[0].astype(np.float64) * (1 - b1 - b2) + tri[1] * b1 + tri[2] * b2
        N = nrm[0].astype(np.float64) * (1 - b1 - b2) + nrm[1] * b1 + nrm[2] * b2
        cosv = (P * N).sum(1) / np.linalg.norm(P, axis=1) / np.linalg.norm(N, axis=1)
        if cls == 2:
            assert (cosv > 0.12 + 1e-3).all(), (tri, nrm, cosv.min())
            closest = min(closest, cosv.min() - 0.12)
        else:
            assert (cosv < 0.12 - 1e-3).all(), (tri, nrm, cosv.max())
            closest = min(closest, 0.12 - cosv.max())
    assert counts[2] > 500 and counts[3] > 500 and counts[0] > 500, counts
    assert closest < 0.02                                      # the classes reach close to the threshold: the bound is not lazy
    for vb, ib, _ in (bunny, dragon):
        from oracle import orc as _o
        h = hostcheck(vb, ib, _o.Scene(vb, ib).bound)
        tp = np.empty((h.T, 12), np.float32)
        L.hc_scene_tripos.argtypes = [C.c_void_p, C.c_void_p]
        L.hc_scene_tripos(h.h, tp.ctypes.data_as(C.c_void_p))
        cls = tp[:, 7].view(np.uint32) >> 28
        assert set(np.unique(cls)) <= {0, 2, 3} and (cls != 0).mean() > 0.7, (cls != 0).mean()   # bunny 0.9, dragon 0.76


def test_parity_row_lists_give_the_oracle_grid(orc, hostcheck, bunny):
    """The parity rule through row lists of the (y, z) plane (pl_rect, dxv_dirmap.h; the device builder and kernel: parity_lists.hip,
    k_parity_rows<.., LISTS>): every triangle whose padded box covers a row's point is in the row's texel, once -- so counting
    over the list equals counting over all triangles.  Host replay against the oracle on the bunny and on lattice-snapped
    adversarial meshes (box edges ON texel borders and row coordinates), coarse and fine grids."""
    import ctypes as C
    from test_fuzz import lattice_mesh
    L = hostcheck.lib
    L.hc_plists_build.argtypes = [C.c_void_p, C.c_uint32]
    L.hc_plists_build.restype = C.c_uint64
    vb, ib, _ = bunny
    s = orc.Scene(vb, ib)
    h = hostcheck(vb, ib, s.bound)
    want = s.voxelize(64, mode=1)
    for R in (64, 512):
        n = L.hc_plists_build(h.h, R)
        assert n >= h.T
        got, _ = h.voxelize(64, mode=13)
        assert np.array_equal(got, want), R
    rng = np.random.default_rng(77)
    for n_tris, Lt, N in ((1, 8, 16), (3, 8, 8), (30, 16, 32), (200, 32, 32), (60, 16, 48)):
        vb, ib = lattice_mesh(rng, n_tris, Lt)
        s = orc.Scene(vb, ib)
        h = hostcheck(vb, ib, s.bound)
        want = s.voxelize(N, mode=1, algo=orc.ALGO_BRUTE)
        for R in (16, 32, 256):                                    # 16, 32: texel borders coincide with lattice coordinates
            L.hc_plists_build(h.h, R)
            got, _ = h.voxelize(N, mode=13)
            assert np.array_equal(got, want), (n_tris, Lt, N, R)


def test_work_queue_brick_test_never_drops_a_live_ray(orc, hostcheck, bunny, dragon):
    """The work queue of the lists kernel (plan_bricks.hip: k_plan_bricks) keeps a 4^3-voxel brick iff dm_box_may_be_live says
    a ray of it can be live -- decided from the brick's hull, three of its corners and a max-mip of the lists' far radii
    (dxv_dirmap.h).  Replayed on the host against the per-voxel first-step decision the kernel makes (origin_leaves_root,
    dm_ray_start: the same functions): no live voxel may sit in a dropped brick, on grids whose bricks straddle the centre
    planes or hang over the grid's end, on slabs and block-cyclic partitions, on coarse and fine maps, on meshes through the
    grid centre -- and the test must stay tight (it is what saves the launch its dead waves)."""
    from test_fuzz import lattice_mesh
    from dxrvoxelizer_amd import meshes
    kept_total = live_total = 0
    for (vb, ib, _), sizes in ((bunny, (64, 100, 50)), (dragon, (128, 66))):
        s = orc.Scene(vb, ib)
        h = hostcheck(vb, ib, s.bound)
        for R in (128, 32):
            h.lists(R)
            # the mip is the maximum over the texels below a cell
            cells = h.lists(R)[0]
            key = np.where((cells[:, 1] & 0xffff) > 0, cells[:, 1] >> 16, 0).astype(np.uint16).reshape(6, R, R)
            mip = h.mip(R)
            off = 0
            for l in range(R.bit_length()):
                r = R >> l
                want = key.reshape(6, r, 1 << l, r, 1 << l).max(axis=(2, 4))
                assert np.array_equal(mip[off:off + 6 * r * r].reshape(6, r, r), want), (R, l)
                off += 6 * r * r
            for N in sizes:
                parts = [(0, N, N, N)]
                if N % 16 == 0:
                    parts += [(N // 4, 10, 10, 10), (N - 6, 6, 6, 6), (4, N // 2, 4, 8), (1, N // 4, 1, 4), (2, N // 2, 2, 4)]
                for z0, nz, zb, zp in parts:
                    live, live_bricks, kept, bad = h.plan_check(N, z0, nz, zb, zp)
                    assert bad == 0, (R, N, z0, nz, zb, zp)
                    assert kept >= live_bricks
                    if zb >= 4 and nz == N and R == 128:
                        kept_total += kept; live_total += live_bricks
    assert kept_total <= 1.40 * live_total, (kept_total, live_total)     # at most two fifths more bricks than hold a live ray (coarse maps, small grids)
    rng = np.random.default_rng(4)
    for n_tris in (1, 3, 30, 200):
        for N in (8, 16, 34):
            vb, ib = lattice_mesh(rng, n_tris, N)
            s = orc.Scene(vb, ib)
            h = hostcheck(vb, ib, s.bound)
            for R in (16, 128):
                h.lists(R)
                assert h.plan_check(N)[3] == 0, (n_tris, N, R)
    vb, ib = meshes.torus(nu=60, nv=30)
    h = hostcheck(vb, ib, orc.Scene(vb, ib).bound)
    h.lists(64)
    live, live_bricks, kept, bad = h.plan_check(96)
    assert bad == 0 and 0 < live_bricks <= kept < (96 // 4) ** 3 // 2     # the torus leaves most of the grid dead
