"""The numpy restatements of the local thickness (tests/thickness_restated.py) held to one another and to what is known in closed form, before
anything of the product is held to them: form (a) by values equals form (b) by openings for both kinds, form (c) per voxel agrees on samples,
slabs, full and empty member sets, symmetries, the two things that are NOT true, the histogram.  No GPU, no library."""
import math

import numpy as np
import pytest

import grid_sides as gs
import morph_restated as mr
import thickness_restated as tr

CASES = [(8, 20), (12, 30), (16, 17)]


def case_grids(N):
    yield from gs.grids(N)
    yield "balls", tr.balls(N, 1)
    yield "complement of balls", (1 - tr.balls(N, 2)).astype(np.uint8)


@pytest.mark.parametrize("N,cap", CASES)
def test_by_values_equals_by_openings_for_both_kinds(N, cap):
    seen = 0
    for name, g in case_grids(N):
        for of in (tr.SOLID, tr.EMPTY):
            a, b = tr.thickness(g, of, cap), tr.thickness_by_openings(g, of, cap)
            assert a.dtype == np.uint32 and np.array_equal(a, b), (N, name, of)
            m = tr.members(g, of)
            assert not a[~m].any() and (a[m] >= 1).all() and (a <= cap).all(), (N, name, of)
            seen += 1
    assert seen == 14


def test_the_per_voxel_form_agrees_on_samples():
    g = tr.balls(16, 5)
    rng = np.random.default_rng(7)
    points = [tuple(p) for p in rng.integers(0, 16, (40, 3))]
    for of in (tr.SOLID, tr.EMPTY):
        W = tr.thickness(g, of, 17)
        assert np.array_equal(tr.thickness_at(g, of, 17, points), np.array([W[p] for p in points], np.uint32)), of


@pytest.mark.parametrize("k", range(1, 8))
def test_a_slab_reads_the_square_of_half_its_thickness_rounded_up(k):
    N = 12
    g = np.zeros((N, N, N), np.uint8)
    g[2:2 + k] = 1
    W = tr.thickness(g, tr.SOLID, 30)
    half = math.ceil(k / 2)
    assert (W[2:2 + k] == half * half).all() and not W[:2].any() and not W[2 + k:].any()
    assert (tr.thickness_voxels(W)[2:2 + k] == 2 * half - 1).all()     # even thicknesses read as the next odd one
    e = tr.thickness(1 - g, tr.EMPTY, 30)                              # the same slab as empty space between two solids
    assert np.array_equal(e, W)


def test_full_and_empty_member_sets():
    full = np.full((8, 8, 8), 0xFF, np.uint8)
    for cap in (2, 20, 4096):
        assert (tr.thickness(full, tr.SOLID, cap) == cap).all()
        assert (tr.thickness(np.zeros_like(full), tr.EMPTY, cap) == cap).all()
        assert not tr.thickness(full, tr.EMPTY, cap).any()
        assert not tr.thickness(np.zeros_like(full), tr.SOLID, cap).any()
    assert np.array_equal(tr.thickness_by_openings(full, tr.SOLID, 12), np.full((8, 8, 8), 12, np.uint32))


def test_the_map_of_a_flipped_or_transposed_grid_is_the_flipped_or_transposed_map():
    g = tr.balls(12, 3)
    for of in (tr.SOLID, tr.EMPTY):
        W = tr.thickness(g, of, 10)
        for axis in (0, 1, 2):
            assert np.array_equal(tr.thickness(np.flip(g, axis), of, 10), np.flip(W, axis)), (of, axis)
        for axes in ((1, 0, 2), (2, 1, 0), (0, 2, 1), (1, 2, 0)):
            assert np.array_equal(tr.thickness(np.transpose(g, axes), of, 10), np.transpose(W, axes)), (of, axes)


def test_discrete_openings_are_not_nested():
    """{ W > r2 } contains OPEN(r2) and does not equal it: here at r2 = 1.  Only { W == cap } == OPEN(cap - 1) is an equality."""
    g = tr.balls(12, 0)
    W = tr.thickness(g, tr.SOLID, 60)
    opened = mr.morph(g, mr.OPEN, 1) != 0
    assert (W[opened] > 1).all()
    assert np.count_nonzero((W > 1) != opened) == 10
    for cap in (2, 3, 5, 9):
        assert np.array_equal(tr.thickness(g, tr.SOLID, cap) == cap, mr.morph(g, mr.OPEN, cap - 1) != 0), cap


def test_the_capped_map_is_not_the_minimum_of_the_uncapped_map_and_the_cap():
    g = tr.balls(12, 0)
    uncapped, capped = tr.thickness(g, tr.SOLID, 60), tr.thickness(g, tr.SOLID, 3)
    assert int(uncapped.max()) < 60
    assert np.count_nonzero(capped != np.minimum(uncapped, 3)) == 2
    assert (capped <= np.minimum(uncapped, 3)).all()


def test_the_histogram_counts_every_voxel_once():
    g = tr.balls(16, 4)
    for of in (tr.SOLID, tr.EMPTY):
        W = tr.thickness(g, of, 17)
        h = tr.histogram(W, 17)
        assert h.dtype == np.uint64 and len(h) == 18 and int(h.sum()) == 16 ** 3
        assert np.array_equal(h, np.bincount(W.reshape(-1), minlength=18))
        assert h.tolist() == [int(np.count_nonzero(W == v)) for v in range(18)]
        assert int(h[0]) == int(np.count_nonzero(~tr.members(g, of)))
