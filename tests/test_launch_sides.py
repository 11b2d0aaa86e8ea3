"""The launch sweep on the CPU (tests/launch_sides.py): the conditions that make its wanted results a test, asserted on the oracle alone at
every side, and the product's host-compiled code against those results at every even side 2 .. 72 -- the half that host and device share
(the walks, the scan of the lists, the closest-hit bodies, the parity rows' clamped blocks, the queue's box test).  With this green, a
device failure of tests/test_gpu_launch_sides.py points at device-only code: store_brick, the clears, the brick order, the launch code."""
import numpy as np
import pytest

import launch_sides as ls
from test_gpu_texels import earlier_scene

REF_WALKS = (0, 2, 6)                    # the stack walk, the four-box walk, the postponed-leaf walk: grid and image
LIST_BODIES = (12, 14)                   # the hit in registers (k_voxelize_queue<true>), the hit in the column (k_voxelize_listed<true>)
PARITY = (1, 3, 4, 7, 8, 10, 11)         # per voxel, with and without the early out; rows 1, 2 x 2, 4 x 4; rows over the four-box nodes


def conditions(orc, w, rules):
    """the conditions of launch_sides.Wanted (asserted where a part is computed), seen to have been asserted; and the earlier scene of the
    device tests, the cube, leaves no zero in grid or image (earlier_scene asserts it) where the wanted image has zeros"""
    N = w.N
    grid, tex = w.ref
    for rule in rules:
        g = grid if rule == "reference" else w.parity
        assert (0 < int(g.sum()) < g.size), (N, rule)
        assert N < 4 or (sorted(w.shares[rule]) == ["x", "y", "z"] and all(0.10 <= s <= 0.90 for s in w.shares[rule].values())), (N, w.shares)
    assert w.tied.shape == (N - ls.overhang(N), N, N) and (w.tied != tex[ls.overhang(N):]).any(), N
    _, _, cube_grid, cube_tex = earlier_scene(orc, N)
    assert cube_grid.all() and cube_tex.all() and (tex == 0).any(), N


@pytest.mark.parametrize("N", ls.SWEEP)
def test_conditions_hold_and_the_bvh_equals_brute_force(orc, N):
    """... and the oracle's BVH, which stands in for brute force at the WIDE sides, gives the same grids and images here, both rules and
    both triangle orders."""
    w = ls.wanted(orc, N)
    assert w.algo == orc.ALGO_BRUTE
    conditions(orc, w, ("reference", "parity"))
    b = ls.Wanted(orc, N, orc.ALGO_BVH)
    for name, got, want in (("grid", b.ref[0], w.ref[0]), ("image", b.ref[1], w.ref[1]), ("parity", b.parity, w.parity), ("tied", b.tied, w.tied)):
        assert np.array_equal(got, want), (N, name)


@pytest.mark.parametrize("N", ls.WIDE)
def test_conditions_hold_at_the_wide_sides(orc, N):
    w = ls.wanted(orc, N)
    assert w.algo == orc.ALGO_BVH
    conditions(orc, w, ("reference", "parity"))


@pytest.mark.parametrize("N", ls.SWEEP)
def test_host_code_equals_the_wanted_results(orc, hostcheck, N):
    """Every walk and every list body with the texel image, the parity modes, and the queue's claim (no live voxel in a brick its box test
    drops) for the whole grid and for the slab (1, N - 1), whose first and last brick layers are both ragged.  And the walk with a column
    of 8 runs out of it at every side: that is what lets the device's redo pass be proven on this mesh."""
    w = ls.wanted(orc, N)
    vb, ib = ls.mesh()
    bound = orc.Scene(vb, ib).bound
    assert np.allclose(bound, [0, 0, 0, 1])
    h = hostcheck(vb, ib, bound)
    for mode in REF_WALKS:
        g, t, ovf = h.voxelize(N, mode, texels=True)
        assert not ovf and np.array_equal(g, w.ref[0]) and np.array_equal(t, w.ref[1]), (N, mode)
    for R in (16, 128):
        h.lists(R)
        for mode in LIST_BODIES:
            g, t, ovf = h.voxelize(N, mode=mode, stack=16, texels=True)
            assert ovf == 0 and np.array_equal(g, w.ref[0]) and np.array_equal(t, w.ref[1]), (N, R, mode)
        for z0, nz in ((0, N), (1, N - 1)):
            live, live_bricks, kept, bad = h.plan_check(N, z0, nz)
            assert bad == 0 and kept >= live_bricks, (N, R, z0, nz, live, live_bricks, kept, bad)
    for mode in PARITY:
        g, ovf = h.voxelize(N, mode)
        assert not ovf and np.array_equal(g, w.parity), (N, mode)
    g, ovf = h.voxelize(N, 0, stack=8)
    assert ovf == 1, N
