"""The numpy restatement of the measures (tests/measure_restated.py) held to facts it does not compute itself: shapes whose Euler characteristic,
faces and moments can be written down, a box's inertia in closed form (also far from the origin, where a float would cancel), record 0 as the
sum of the others, the thin's own Euler number, the grid's symmetries, and the Betti numbers of a ball, a torus, a shell and two linked
rings.  No GPU, no library."""
import itertools

import numpy as np
import pytest

import components_restated as cr
import fill_restated as fr
import grid_sides as gs
import measure_restated as ms
import thin_restated as tr
import thin_shapes as ts

BOTH = (6, 26)


def box(N, lo, hi):
    """solid voxels lo[a] .. hi[a] - 1 along (x, y, z)"""
    g = np.zeros((N, N, N), np.uint8)
    g[lo[2]:hi[2], lo[1]:hi[1], lo[0]:hi[0]] = 1
    return g


def tunnelled(crossing):
    g = box(14, (2, 2, 2), (11, 11, 11))
    g[6, 6, 2:11] = 0                                                   # a through tunnel along x
    if crossing:
        g[8, 2:11, 6] = 0                                               # ... and one along y that crosses over it, two voxels higher: two handles
    return g


def linked_rings():
    g = np.zeros((24, 24, 24), np.uint8)
    g[10, 4:15, 4:15] = 1
    g[10, 5:14, 5:14] = 0                                               # a square ring in the plane z = 10 round (9, 9) ...
    ring = np.zeros((24, 24), np.uint8)                                 # ... and one in the plane y = 9 through its middle: [z, x]
    ring[5:16, 9:20] = 1
    ring[6:15, 10:19] = 0
    assert not (g[:, 9, :] & ring).any()
    g[:, 9, :] |= ring
    return g


SHAPES = [("box", lambda: box(12, (2, 3, 1), (6, 8, 7)), 1), ("hollow box", lambda: gs.hollow_box(12, 2, 8), 2), ("one tunnel", lambda: tunnelled(False), 0),
          ("two crossing tunnels", lambda: tunnelled(True), -1), ("torus 32", lambda: ts.torus(32), 0), ("all solid", lambda: ts.full(10), 1)]


@pytest.mark.parametrize("name,make,chi", SHAPES, ids=[s[0] for s in SHAPES])
def test_euler_of_shapes_whose_answer_can_be_written_down(name, make, chi):
    g = make()
    for conn in BOTH:
        t = ms.measure(g, cr.SOLID, conn)
        assert len(t) == 2 and t["euler"].tolist() == [chi, chi], (name, conn)
        assert t[0]["voxels"] == np.count_nonzero(g)
    assert tr.euler(g) == chi


def test_two_voxels_touching_at_a_corner():
    g = np.zeros((4, 4, 4), np.uint8)
    g[1, 1, 1] = g[2, 2, 2] = 1
    t = ms.measure(g, cr.SOLID, 26)
    assert len(t) == 2 and t[1]["euler"] == 1 and t[1]["voxels"] == 2 and t[1]["faces"] == 12      # 27 + 27 - 1 corners ... : one contractible piece
    t = ms.measure(g, cr.SOLID, 6)
    assert len(t) == 3 and t["euler"].tolist() == [2, 1, 1]


def box_record(lo, hi):
    """the record of the box lo .. hi - 1 by closed forms"""
    n = [hi[a] - lo[a] for a in range(3)]
    V = n[0] * n[1] * n[2]
    s1 = [sum(range(lo[a], hi[a])) for a in range(3)]
    s2 = [sum(i * i for i in range(lo[a], hi[a])) for a in range(3)]
    rec = np.zeros(1, ms.RECORD)[0]
    rec["voxels"] = V
    for a in range(3):
        rec["sum"][a] = s1[a] * V // n[a]
        rec["sum2"][a] = s2[a] * V // n[a]
        b = (a + 1) % 3
        rec["prod"][a] = s1[a] * s1[b] * V // (n[a] * n[b])
    rec["faces"] = 2 * (n[0] * n[1] + n[1] * n[2] + n[2] * n[0])
    rec["euler"] = 1
    return rec


@pytest.mark.parametrize("N,lo,hi", [(12, (2, 3, 1), (6, 8, 7)), (16, (0, 0, 0), (16, 16, 16)), (194, (189, 187, 190), (194, 194, 194))])
def test_a_box_has_its_closed_forms_and_its_inertia_exactly(N, lo, hi):
    from dxrvoxelizer_amd import mass_properties
    g = box(N, lo, hi)
    labelling = (g.astype(np.uint32), 1)                                # one component: its labels are the grid
    a, b, c = (hi[i] - lo[i] for i in range(3))
    for conn in BOTH:
        t = ms.measure(g, cr.SOLID, conn, labelling)
        want = box_record(lo, hi)
        assert t[0] == want and t[1] == want, conn
        mp = mass_properties(t)
        V = a * b * c
        assert mp["volume"].tolist() == [V, V] and mp["area"].tolist() == [2 * (a * b + b * c + c * a)] * 2
        assert mp["centroid"][1].tolist() == [(lo[i] + hi[i]) / 2 for i in range(3)]
        assert mp["inertia"][1].tolist() == np.diag([V * (b * b + c * c) / 12, V * (c * c + a * a) / 12, V * (a * a + b * b) / 12]).tolist()


def test_mass_properties_products_of_inertia_and_the_empty_record():
    from dxrvoxelizer_amd import MEASURE_RECORD, mass_properties
    assert MEASURE_RECORD == ms.RECORD
    g = np.zeros((8, 8, 8), np.uint8)
    g[1, 2, 3] = g[5, 6, 4] = 1                                         # two voxels: (3, 2, 1) and (4, 6, 5)
    mp = mass_properties(ms.measure(g, cr.SOLID, 26, (g.astype(np.uint32), 1)))
    d = np.array([0.5, 2.0, 2.0])                                       # each voxel's offset from the centroid, +-
    want = 2 * (d @ d * np.eye(3) - np.outer(d, d)) + 2 * np.eye(3) / 6
    assert np.allclose(mp["inertia"][0], want, rtol=1e-14, atol=0) and mp["centroid"][0].tolist() == [4.0, 4.5, 3.5]
    none = mass_properties(ms.measure(np.zeros((4, 4, 4), np.uint8)))
    assert none["volume"].tolist() == [0] and np.isnan(none["centroid"]).all() and not none["inertia"].any()


@pytest.mark.parametrize("N", [2, 10, 64])
def test_an_all_solid_grid_has_six_faces_of_n_squared(N):
    for conn in BOTH:
        t = ms.measure(ts.full(N), cr.SOLID, conn)
        assert t["faces"].tolist() == [6 * N * N] * 2 and t["euler"].tolist() == [1, 1] and t[0]["voxels"] == N ** 3


def test_the_empty_space_of_a_hollow_box_under_6():
    t = ms.measure(gs.hollow_box(12, 2, 8), cr.EMPTY, 6)
    assert len(t) == 3 and t["euler"].tolist() == [3, 2, 1]             # the outside, a box with a box-shaped hole; the inside
    assert t[2]["voxels"] == 5 ** 3 and t[2]["faces"] == 6 * 25
    assert ms.measure(np.ones((4, 4, 4), np.uint8), cr.EMPTY, 6).tobytes() == bytes(96)             # K = 0: one all-zero record


@pytest.mark.parametrize("N", [12, 20, 34])
def test_record_0_is_the_sum_and_equals_the_thins_euler_number(N):
    g = fr.random_walls(N, 0.3, N, bytes_other_than_one=True)
    for of, conn in itertools.product((cr.SOLID, cr.EMPTY), BOTH):
        t = ms.measure(g, of, conn)
        assert len(t) > 2 or (of, conn) != (cr.SOLID, 6)
        for name in ms.RECORD.names:
            assert np.array_equal(t[name][0], t[name][1:].sum(axis=0)), (name, of, conn)
        assert t[0]["voxels"] == np.count_nonzero(cr.members(g, of))
    assert ms.measure(g, cr.SOLID, 26)[0]["euler"] == tr.euler(g)
    assert np.array_equal(ms.measure(g, cr.SOLID, 26)[["voxels", "sum", "sum2", "prod", "faces"]][0], ms.measure(g, cr.SOLID, 6)[["voxels", "sum", "sum2", "prod", "faces"]][0])


def test_thinning_to_the_kernel_leaves_the_euler_number():
    g = fr.random_walls(24, 0.3, 24)
    before = ms.measure(g, cr.SOLID, 26)
    after = ms.measure(tr.thin(g, tr.KERNEL)[0], cr.SOLID, 26)
    assert before[0]["euler"] == after[0]["euler"] and len(before) == len(after) and before[0]["euler"] < 0


def per_component(t):
    return sorted(zip(t["voxels"][1:].tolist(), t["faces"][1:].tolist(), t["euler"][1:].tolist()))


def test_flips_and_permutations_move_the_moments_and_nothing_else():
    N = 20
    g = fr.random_walls(N, 0.3, 5)
    for of, conn in itertools.product((cr.SOLID, cr.EMPTY), BOTH):
        t = ms.measure(g, of, conn)
        for fx, fy, fz in itertools.product((False, True), repeat=3):
            f = g[::-1 if fz else 1, ::-1 if fy else 1, ::-1 if fx else 1]
            tf = ms.measure(f, of, conn)
            assert per_component(tf) == per_component(t)
            assert tf[0] == ms.mirrored(t[:1], N, (fx, fy, fz))[0], (of, conn, fx, fy, fz)
        for axes in itertools.permutations(range(3)):
            tp = ms.measure(g.transpose(axes), of, conn)
            assert per_component(tp) == per_component(t)
            assert tp[0] == ms.permuted(t[:1], axes)[0], (of, conn, axes)
    assert ms.measure(g, cr.SOLID, 6)[0]["sum"].tolist() != ms.measure(g[:, :, ::-1], cr.SOLID, 6)[0]["sum"].tolist()


def betti(g):
    from dxrvoxelizer_amd import betti_numbers
    _, empty = cr.label(g, cr.EMPTY, 6)
    t = ms.measure(g, cr.SOLID, 26)
    return betti_numbers(len(t) - 1, np.count_nonzero((empty["flags"] & 1) == 0), t[0]["euler"])


def test_betti_numbers_of_ball_torus_shell_and_linked_rings():
    assert betti(ts.ball(20)) == (1, 0, 0)
    assert betti(ts.torus(32)) == (1, 1, 0)
    assert betti(ts.shell(20)) == (1, 0, 1)
    assert betti(linked_rings()) == (2, 2, 0)
    assert betti(gs.hollow_box(12, 1, 10)) == (1, 0, 1)
