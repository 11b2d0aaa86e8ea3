"""The restatements of the access radius and the intrusion map (tests/access_restated.py) against one another: the widest-path search == the
threshold form, the definition of I == the erode / keep-connected / dilate loop, on every builder, both kinds, both connectivities and the
three kinds of seeds; and the properties include/dxv.h lists under the rule.  Pure numpy and scipy: no library, no GPU."""
import numpy as np
import pytest

import access_restated as ar
import geodesic_restated as gr
import thickness_restated as tr

BUILDERS = ar.builders()
CAP = 9                                                                  # every builder has radii below and at it


def seedings(g, listed):
    rng = np.random.default_rng(5)
    return (("border", "border"), ("list", np.array(listed, np.uint32)), ("mask", (rng.random(g.shape) < 0.02).astype(np.uint8) * 0x40))


@pytest.mark.parametrize("name", [b[0] for b in BUILDERS])
def test_the_forms_agree_and_the_properties_hold(name):
    _, g, listed = next(b for b in BUILDERS if b[0] == name)
    for of in (ar.SOLID, ar.EMPTY):
        R = ar.radius(g, of, CAP)
        W = tr.thickness(g, of, CAP)
        for connectivity in (6, 26):
            for kind, seeds in seedings(g, listed):
                key = (name, of, connectivity, kind)
                A = ar.access(g, of, connectivity, CAP, seeds)
                assert A.tobytes() == ar.access_by_thresholds(g, of, connectivity, CAP, seeds).tobytes(), key
                I = ar.intrusion(g, of, A)
                assert I.tobytes() == ar.intrusion_by_loop(g, of, connectivity, CAP, seeds).tobytes(), key
                reached = A > 0
                assert (A <= R).all() and (A[reached] <= I[reached]).all() and (I <= W).all() and not I[~reached].any(), key
                S = ar.seed_mask(g.shape, seeds) & ar.members(g, of)
                assert np.array_equal(A[S], R[S].astype(np.uint32)), key       # on seeds A = R
                G = gr.geodesic_dijkstra(g, of, gr.FACES if connectivity == 6 else gr.CHAMFER, seeds)
                assert np.array_equal(reached, G < gr.UNREACHED), key
                t = ar.tally(g, of, A, seeds)
                assert t["seeds_used"] == int(S.sum()) and t["reached"] + t["unreached"] == int(ar.members(g, of).sum()), key


@pytest.mark.parametrize("name", ["bottle 3", "random 0.3"])
def test_the_cap_identity_holds_for_a_and_not_for_i(name):
    _, g, _ = next(b for b in BUILDERS if b[0] == name)
    differs = False
    for of in (ar.SOLID, ar.EMPTY):
        full = ar.access(g, of, 26, 4096)
        for cap in (2, 5, 65):
            A = ar.access(g, of, 26, cap)
            assert np.array_equal(A, np.minimum(full, cap)), (name, of, cap)
            differs |= not np.array_equal(ar.intrusion(g, of, A), np.minimum(ar.intrusion(g, of, full), cap))
    assert differs or name != "bottle 3"                                # a ball of the larger cap covers voxels no ball of the smaller one does


def test_with_every_member_a_seed_it_is_the_radius_and_the_thickness():
    _, g, _ = next(b for b in BUILDERS if b[0] == "random 0.3")
    for of in (ar.SOLID, ar.EMPTY):
        for cap in (9, 4096):
            A = ar.access(g, of, 6, cap, np.ones(g.shape, np.uint8))
            assert np.array_equal(A, ar.radius(g, of, cap)) and ar.intrusion(g, of, A).tobytes() == tr.thickness(g, of, cap).tobytes()


def test_the_builders_are_what_they_say():
    g, channel, chamber = ar.ink_bottle(16, 1)
    assert ar.radius(g, ar.EMPTY, 4096)[channel] == 1 and ar.radius(g, ar.EMPTY, 4096)[chamber] == 16 and ar.access(g, ar.EMPTY, 6, 4096)[chamber] == 1
    g, channel, chamber = ar.ink_bottle(16, 3)
    assert ar.radius(g, ar.EMPTY, 4096)[channel] == 4 and ar.access(g, ar.EMPTY, 6, 4096)[chamber] == 4
    for shift in range(8):
        for sx, sz in ((shift, 0), (0, shift)):
            g, channel, chamber = ar.ink_bottle(24, 1, sx, sz)
            assert g.shape == (24, 24, 24) and g[chamber] == 0 and g[channel] == 0 and ar.access(g, ar.EMPTY, 6, 65)[chamber] == 1
    g, seed, chamber = ar.raised_twice()
    A = ar.access(g, ar.EMPTY, 6, 4096, np.array([seed]))
    assert A[chamber] == 4 and ar.radius(g, ar.EMPTY, 4096)[chamber] == 9 and A[3, 10, 3] == 1 and g.reshape(-1)[seed] == 0
    g = ar.staircase()
    assert int((ar.access(g, ar.EMPTY, 6, 4096) > 0).sum()) == 1 and int((ar.access(g, ar.EMPTY, 26, 4096) > 0).sum()) == int((g == 0).sum())
