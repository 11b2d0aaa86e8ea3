"""The conditions of the unsettled-operator matrix (tests/unsettled_cases.py) on the host libraries alone, at both sides: what the device test
(tests/test_gpu_unsettled.py) compares with could tell a finished leader from an unfinished one, for every pair, for the chain four deep, for
the three frames, for the wide side's diagonal; the leaders take what the matrix was laid out for; the restatements give what the host
libraries give; and a grid that meets no condition is refused."""
import numpy as np
import pytest

import fill_host as fh
import unsettled_cases as uc

# what the host libraries say of the leaders on the matrix' grid: {side: (fill rounds, voxels filled, thin iterations, voxels removed, of them in the
# first iteration, the geodesic's host rounds and unreached voxels, the access' host rounds and unreached voxels)}
LAID_OUT_FOR = {22: (5, 310, 10, 3792, 2590, 7, 0, 10, 58), 66: (10, 10030, 18, 98600, 58709, 13, 0, 27, 922)}


@pytest.mark.parametrize("N", [uc.SIDE, uc.WIDE_SIDE])
def test_the_leaders_take_what_the_matrix_was_laid_out_for(N):
    g = uc.grid(N)
    fill, thin = uc.leader("fill", g), uc.leader("thin", g)
    first = uc.th.thin(g, uc.CURVE, 1)
    geodesic, access = uc.flood_report("geodesic", g), uc.flood_report("access", g)
    got = (fill.report["rounds"], int(np.count_nonzero(fill.after)) - int(np.count_nonzero(g)), thin.report["thin_info"][0], thin.report["thin_info"][1], first[2],
           geodesic[1], geodesic[0]["tally"]["unreached"], access[1], access[0]["tally"]["unreached"])
    assert got == LAID_OUT_FOR[N]
    assert thin.report["thin_info"][1] == int(np.count_nonzero(g)) - int(np.count_nonzero(thin.after))


@pytest.mark.parametrize("name", uc.LEADERS)
@pytest.mark.parametrize("N", [uc.SIDE, uc.WIDE_SIDE])
def test_every_pair_meets_its_conditions(N, name):
    g = uc.grid(N)
    cells = 0
    for follower in uc.FOLLOWERS:
        lead, w, again = uc.pair(name, follower, g)
        assert lead.name == name and (again is None) == (follower in uc.PLAIN_FOLLOWERS)
        cells += 1
    assert cells * len(uc.LEADERS) == uc.CELLS == 280


def test_the_excuses_are_the_ones_written_down():
    """an editor whose edit changes nothing on a leader's grid is excused by name and reason, and nobody else is: whoever is excused does change nothing"""
    g = uc.grid(uc.SIDE)
    for name in uc.LEADERS:
        for follower in uc.EDITORS:
            lead, w, _ = uc.pair(name, follower, g)
            assert bool(uc.excused(name, follower)) == bool(np.array_equal(w["grid"], lead.after)), (name, follower)


def test_the_chain_four_deep_and_the_three_frames():
    fill, thin, geodesic, access, sight = uc.four_deep(uc.grid(uc.SIDE))
    assert np.array_equal(thin.before, fill.after) and geodesic.before is thin.after and access.before is thin.after
    assert sight["tally"]["members"] == int(np.count_nonzero(thin.after == 0))
    assert len({uc.grid(N).shape for N in uc.FRAME_SIDES}) == 3
    for N, name, follower in uc.FRAMES:
        uc.pair(name, follower, uc.grid(N))
    assert len({name for _, name, _ in uc.FRAMES}) == 3


def test_the_diagonal_at_the_wide_side():
    g = uc.grid(uc.WIDE_SIDE)
    for name, followers in uc.DIAGONAL.items():
        for follower in followers:
            uc.pair(name, follower, g)


@pytest.mark.parametrize("name", uc.LEADERS)
def test_the_restatements_give_what_the_host_libraries_give(name):
    """on the grid each leader leaves at the small side: the device test compares with the host libraries, and through them with these"""
    after = uc.leader(name, uc.grid(uc.SIDE)).after
    seen = 0
    for follower in uc.RESTATED:
        w = uc.want(follower, after)
        for what, value in uc.restated(follower, np.array(after)).items():
            assert uc.same(value, w[what]) or (what == "tally" and all(value[k] == w[what][k] for k in value)), (name, follower, what)
            seen += 1
    assert seen >= len(uc.RESTATED) + 10


def test_a_grid_that_meets_no_condition_is_refused(monkeypatch):
    """flipped by hand: a grid the fill finishes in its first rounds, a thin that is over at once, a flood that stays at home, a follower that
    cannot tell one grid from another"""
    N = uc.SIDE
    box = np.zeros((N, N, N), np.uint8)
    box[4:12, 4:12, 4:12] = 1                                           # nothing enclosed, nothing far from the border
    assert fh.fill(box)[1] < uc.MIN_ROUNDS
    with pytest.raises(AssertionError, match="fill: . rounds"):
        uc.leader("fill", box)
    with pytest.raises(AssertionError, match="thin: . iterations|the first iteration alone"):
        one = np.zeros((N, N, N), np.uint8)
        one[3, 3, 3] = 1
        uc.leader("thin", one)
    with pytest.raises(AssertionError, match="stays within"):
        near = np.zeros((N, N, N), np.uint8)
        near[0:6, 0:6, 0:6] = 1                                         # a flood that never leaves the seed's tile
        near[0:6, 0, 0:8] = 1
        uc.leader("geodesic", near)
    blind = lambda follower, g: {"grid": g, "count": 7}                   # a count that does not look at the grid
    g = uc.fr.random_walls(N, uc.DENSITY, 12345)                          # (a grid nobody has a wanted result of)
    monkeypatch.setattr(uc, "_host", blind)
    try:
        with pytest.raises(AssertionError, match="fill -> count: the same result on the grid before"):
            uc.pair("fill", "count", g)
    finally:
        for k in [k for k in uc._WANT if k[-1] == "count" and uc._WANT[k]["count"] == 7]:
            del uc._WANT[k]
