"""The two numpy restatements of the maximal-ball partition (tests/partition_restated.py) held to each other -- (a) vectorised == (b) the
definition read voxel by voxel -- and to hand cases whose answer is known without either.  No GPU, no product code."""
import numpy as np
import pytest

import partition_restated as pr


def rows(table):
    return [tuple(v.tolist() for v in rec) for rec in table]


def same(A, B):
    return all(np.asarray(a).dtype == np.asarray(b).dtype and np.asarray(a).tobytes() == np.asarray(b).tobytes() for a, b in zip(A, B))


@pytest.mark.parametrize("N,density,seed", [(6, 0.5, 0), (8, 0.6, 1), (8, 0.3, 2), (10, 0.8, 3), (12, 0.7, 4)])
def test_the_vectorised_form_equals_the_literal_one(N, density, seed):
    g = pr.noise(N, density, seed)
    for of in (pr.SOLID, pr.EMPTY):
        for cap in (1, 2, 5, 4096) if N < 12 else (5,):
            a, b = pr.partition(g, of, cap), pr.partition_literal(g, of, cap)
            assert same(a, b[:3]), (N, of, cap)
            assert np.array_equal(pr.parents(pr.radius(g, of, cap)), b[3]), (N, of, cap)


def test_a_blob_on_a_small_grid_both_ways():
    g = pr.balls(12, 5, count=4, rmax=4)
    for of in (pr.SOLID, pr.EMPTY):
        assert same(pr.partition(g, of, 17), pr.partition_literal(g, of, 17)[:3]), of


def test_a_full_grid_is_one_region_rooted_at_voxel_0():
    labels, table, throats = pr.partition(np.ones((16, 16, 16), np.uint8), pr.SOLID, 16)
    assert (labels == 1).all() and len(throats) == 0
    assert rows(table) == [(0, 16, 4096, 0, [0, 0, 0], [15, 15, 15], 1)]


def test_the_dumbbell():
    g = pr.dumbbell()
    for cap in (4096, 16):
        labels, table, throats = pr.partition(g, pr.SOLID, cap)
        big = table[table["voxels"] > 1]
        assert sorted(big["voxels"].tolist()) == [934, 1430] and int((table["voxels"] == 1).sum()) == 4, cap
        assert int(table["voxels"].sum()) == int(g.sum())
        if cap == 4096:
            assert big["radius_sq"].tolist() == [50, 37]
            assert table["radius_sq"][table["voxels"] == 1].tolist() == [1, 1, 1, 1]
    labels, table, throats = pr.partition(g, pr.SOLID, 4096)
    a, b = (int(k) + 1 for k in np.flatnonzero(table["voxels"] > 1))
    between = throats[(throats["a"] == a) & (throats["b"] == b)]
    R = pr.radius(g, pr.SOLID, 4096)
    assert len(between) == 1 and int(between["neck_sq"][0]) == int(R[16, 16, 16]) == 5      # the bar's axis: the nearest empty voxel is (2, 1) away
    assert int(between["faces"][0]) == 13                               # the bar's cross-section, |d|^2 <= 4
    net = pr.pore_network(table, throats)
    assert net["coordination"].tolist() == table["throats"].tolist() and abs(net["neck_radius"][-1] - 5 ** 0.5) < 1e-12


def test_an_all_empty_grid_has_no_solid_region_and_one_corner_voxel_is_one_region():
    empty = np.zeros((8, 8, 8), np.uint8)
    labels, table, throats = pr.partition(empty, pr.SOLID, 17)
    assert not labels.any() and len(table) == 0 and len(throats) == 0
    labels, table, throats = pr.partition(empty, pr.EMPTY, 17)
    assert (labels == 1).all() and rows(table) == [(0, 17, 512, 0, [0, 0, 0], [7, 7, 7], 1)]
    empty[7, 7, 7] = 3
    labels, table, throats = pr.partition(empty, pr.SOLID, 17)
    assert int(labels.sum()) == 1 and labels[7, 7, 7] == 1 and len(throats) == 0
    assert rows(table) == [(511, 1, 1, 0, [7, 7, 7], [7, 7, 7], 1)]


@pytest.mark.parametrize("of", [pr.SOLID, pr.EMPTY])
def test_the_forest_properties(of):
    g = pr.balls(24, 9, count=6, rmax=6)
    N = 24
    R = pr.radius(g, of, 26).reshape(-1)
    parent = pr.parents(R.reshape(N, N, N))
    root = pr.roots(parent)
    member = R > 0
    assert np.array_equal(parent != pr.NONE, member)
    at = np.flatnonzero(member)
    up = parent[at].astype(np.int64)
    d2 = (up % N - at % N) ** 2 + (up // N % N - at // N % N) ** 2 + (up // (N * N) - at // (N * N)) ** 2
    assert (d2 <= R[at]).all()                                          # every parent lies in its voxel's closed ball
    moved = up != at
    assert ((R[up] > R[at]) | ((R[up] == R[at]) & (up < at)))[moved].all()     # ... and strictly above it
    r = root[at].astype(np.int64)
    assert (parent[r] == r).all()                                       # every member's root is a root
    labels, table, _ = pr.partition(g, of, 26)
    assert (np.diff(table["root"].astype(np.int64)) > 0).all()          # the labels of roots ascend with their indices
    assert np.array_equal(labels.reshape(-1)[table["root"]], np.arange(1, len(table) + 1))
    assert np.array_equal(table["radius_sq"], R[table["root"]])


def test_the_prototype_counts():
    """what the rule gave when it was first tried at 32^3: properties of the rule, written down"""
    t = pr.partition(pr.torus(), pr.SOLID, 4096)[1]
    assert int(t["voxels"].sum()) == int(pr.torus().sum()) and len(t) >= 4      # a tube of constant width is cut into arcs
    z, y, x = np.indices((32, 32, 32))
    cyl = (((z - 16) ** 2 + (y - 16) ** 2 <= 16) & (x >= 4) & (x <= 27)).astype(np.uint8)
    t = pr.partition(cyl, pr.SOLID, 4096)[1]
    assert len(t) >= 2 and int(t["voxels"].sum()) == int(cyl.sum())
