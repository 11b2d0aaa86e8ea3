"""The two restatements of the geodesic distance (tests/geodesic_restated.py) held to each other and to cases worked out by hand: (a) the numpy
relaxation == (b) Dijkstra on small grids for both kinds, both metrics, border seeds and a single seed; the limit's two forms; a straight
corridor; one diagonal and one corner step; the 3-D checkerboard; a sealed cavity; the tally and the path of a case small enough to read.  No GPU,
nothing of the product."""
import numpy as np
import pytest

import geodesic_restated as gr
import grid_sides as gs

U, X = gr.UNREACHED, gr.NONE


@pytest.mark.parametrize("N", [2, 6, 10, 18, 24])
def test_relaxation_equals_dijkstra(N):
    for name, g in gs.grids(N):
        for of in (gr.SOLID, gr.EMPTY):
            for metric in (gr.FACES, gr.CHAMFER):
                for seeds in ("border", gr.smallest_member(g, of)):
                    a, b = gr.geodesic(g, of, metric, seeds), gr.geodesic_dijkstra(g, of, metric, seeds)
                    assert a.dtype == np.uint32 and a.tobytes() == b.tobytes(), (N, name, of, metric)
                    assert np.array_equal(a == X, ~gr.members(g, of))


def test_the_three_ways_to_give_seeds_agree():
    g = dict(gs.grids(10))["random 0.3"]
    idx = np.array([5, 5, 17, 999, 123], np.uint32)                      # a duplicate among them
    mask = np.zeros(1000, np.uint8)
    mask[idx] = 7
    for metric in (gr.FACES, gr.CHAMFER):
        a = gr.geodesic(g, gr.EMPTY, metric, idx)
        assert a.tobytes() == gr.geodesic(g, gr.EMPTY, metric, mask.reshape(10, 10, 10)).tobytes() == gr.geodesic_dijkstra(g, gr.EMPTY, metric, idx).tobytes()
        assert gr.tally(a)["seeds_used"] == int(gr.members(g, gr.EMPTY).reshape(-1)[[5, 17, 999, 123]].sum())


@pytest.mark.parametrize("metric", [gr.FACES, gr.CHAMFER])
def test_the_limit_two_ways(metric):
    g = gr.serpentine(16)
    seeds = gr.smallest_member(g, gr.SOLID)
    out0 = gr.geodesic(g, gr.SOLID, metric, seeds)
    far = gr.tally(out0)["farthest"]
    occurring = int(np.unique(out0[out0 < U])[7])
    for limit in (1, occurring, far // 2, far, far + 10):
        direct = gr.geodesic(g, gr.SOLID, metric, seeds, limit)
        assert direct.tobytes() == gr.limited(out0, limit).tobytes() == gr.geodesic_dijkstra(g, gr.SOLID, metric, seeds, limit).tobytes(), limit
        members = out0 != X
        assert np.array_equal(direct[members], np.where(out0[members] <= limit, out0[members], U))
        assert (direct == limit).any() == (out0 == limit).any()         # a voxel with G == limit is kept
    assert (gr.limited(out0, occurring) == occurring).any()
    assert gr.limited(out0, 0) is out0


def test_a_straight_corridor_counts_its_steps():
    g = gr.corridor(12, 9)
    seed = np.array([(1 * 12 + 1) * 12 + 1], np.uint32)
    assert gr.geodesic(g, gr.SOLID, gr.FACES, seed)[1, 1, 1:10].tolist() == list(range(9))
    assert gr.geodesic(g, gr.SOLID, gr.CHAMFER, seed)[1, 1, 1:10].tolist() == list(range(0, 27, 3))
    assert gr.tally(gr.geodesic(g, gr.SOLID, gr.CHAMFER, seed)) == {"seeds_used": 1, "reached": 9, "unreached": 0, "farthest": 24, "farthest_voxel": (1 * 12 + 1) * 12 + 9}


def test_one_diagonal_step_costs_4_and_one_corner_step_5():
    g = np.zeros((4, 4, 4), np.uint8)
    g[1, 1, 1] = g[1, 2, 2] = g[2, 3, 3] = 1                            # seed, an edge neighbour of it, a corner neighbour of that
    seed = np.array([(1 * 4 + 1) * 4 + 1], np.uint32)
    out = gr.geodesic(g, gr.SOLID, gr.CHAMFER, seed)
    assert (out[1, 1, 1], out[1, 2, 2], out[2, 3, 3]) == (0, 4, 9)
    faces = gr.geodesic(g, gr.SOLID, gr.FACES, seed)
    assert (faces[1, 1, 1], faces[1, 2, 2], faces[2, 3, 3]) == (0, U, U)
    # a step squeezes between two solid voxels of the other kind without asking: the empty space's diagonal through a solid pair
    h = np.ones((2, 2, 2), np.uint8)
    h[0, 0, 0] = h[0, 1, 1] = 0
    assert gr.geodesic(h, gr.EMPTY, gr.CHAMFER, np.array([0], np.uint32))[0, 1, 1] == 4


def test_the_checkerboard():
    g = gr.checkerboard(10)
    seed = np.array([0], np.uint32)
    faces = gr.geodesic(g, gr.SOLID, gr.FACES, seed)
    assert faces[0, 0, 0] == 0 and np.count_nonzero(faces == U) == 499 and np.count_nonzero(faces == X) == 500
    chamfer = gr.geodesic(g, gr.SOLID, gr.CHAMFER, seed)
    assert not (chamfer == U).any() and chamfer[g != 0].max() == 4 * 13     # edge steps only (a corner step lands on the other colour): (9, 9, 8) takes (9 + 9 + 8) / 2 of them
    t = gr.tally(chamfer)
    assert (t["reached"], t["unreached"], t["seeds_used"]) == (500, 0, 1)


def test_a_sealed_cavity_is_unreached_from_the_border():
    g = gr.sealed_cavity(16)
    for metric in (gr.FACES, gr.CHAMFER):
        out = gr.geodesic(g, gr.EMPTY, metric, "border")
        inside = np.zeros(g.shape, bool)
        inside[5:11, 5:11, 5:11] = True
        assert np.array_equal(out == U, inside) and gr.tally(out)["unreached"] == 6 ** 3
        assert out[0, 3, 3] == 0 and out[3, 3, 3] == 3 * (1 if metric == gr.FACES else 3)


def test_nothing_reached():
    g = np.ones((4, 4, 4), np.uint8)
    out = gr.geodesic(g, gr.EMPTY, gr.FACES, "border")
    assert (out == X).all() and gr.tally(out) == {"seeds_used": 0, "reached": 0, "unreached": 0, "farthest": 0, "farthest_voxel": 0xFFFFFFFF}
    out = gr.geodesic(g, gr.SOLID, gr.FACES, np.zeros(0, np.uint32))
    assert (out == U).all() and gr.tally(out)["unreached"] == 64 and gr.tally(out)["farthest_voxel"] == 0xFFFFFFFF
    assert gr.geodesic_dijkstra(g, gr.SOLID, gr.FACES, np.zeros(0, np.uint32)).tobytes() == out.tobytes()


def test_the_path_takes_the_first_neighbour_in_index_order():
    g = np.ones((3, 3, 3), np.uint8)
    out = gr.geodesic(g, gr.SOLID, gr.FACES, np.array([0], np.uint32))
    p = gr.path(out, gr.FACES, 26)
    assert p.tolist() == [26, 17, 8, 5, 2, 1, 0]                        # -z first, then -y, then -x
    gr.check_path(out, gr.FACES, p, 26)
    out = gr.geodesic(g, gr.SOLID, gr.CHAMFER, np.array([0], np.uint32))
    assert gr.path(out, gr.CHAMFER, 26).tolist() == [26, 13, 0] and out[2, 2, 2] == 10
    assert gr.path(out, gr.CHAMFER, 0).tolist() == [0]
