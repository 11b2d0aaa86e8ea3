"""The numbering that components.hip and skeleton.hip share (csrc/dxv_label.h) where its two kinds of root meet: grids of side 6 and 10 -- 216 and
1000 voxels, neither a multiple of 64 -- of isolated voxels (one node each) and bars of three voxels along x (a node, a one-voxel branch, a
node), every second row in y and z so that no two features touch.  The roots are then single voxels side by side: every bar puts a node root, a
branch root and a node root into consecutive bits, most 64-voxel words of the linear order hold roots of both kinds, and the bar on voxels
63, 64, 65 is a run of roots that crosses a word boundary with a root of either kind on either side of it.  The host routines say so before
the device is asked: dxv_skeleton's labels and tables equal tests/skeleton_host.py byte for byte, and the same grid under
dxv_components(SOLID, 26) equals tests/components_host.py."""
import numpy as np
import pytest

import components_host as ch
import skeleton_host as sh
from raycast_restated import write_grid

BRANCH = 0x80000000


def pattern(N):
    """[N, N, N] uint8: the bar on voxels 63 .. 65 with an isolated voxel in front of it, and in every second row of its parity alternating
    isolated voxels and bars"""
    g = np.zeros((N, N, N), np.uint8)
    row, x = divmod(63, N)
    assert x == 3
    y0, z0 = row % N, row // N
    for z in range(z0 % 2, N, 2):
        for y in range(y0 % 2, N, 2):
            if (y, z) == (y0, z0):
                g[z, y, 1] = 1
                g[z, y, 3:6] = 1
                g[z, y, 7:N:2] = 1
            elif (y // 2 + z // 2) % 2:
                g[z, y, 0:3] = 1
                g[z, y, 4] = 1
                if N >= 9:
                    g[z, y, 6:9] = 1
            else:
                g[z, y, 0] = 1
                g[z, y, 2:5] = 1
                g[z, y, 6:N:2] = 1
    return g


def roots(nodes, branches, N):
    """(node roots, branch roots) as sets of linear indices: a record's `first` is its root"""
    return {int(f) for f in nodes["first"]}, {int(f) for f in branches["first"]}


@pytest.mark.parametrize("N", (6, 10))
def test_the_pattern_has_a_mixed_word_and_a_run_of_roots_across_a_word_boundary(N):
    g = pattern(N)
    labels, nodes, branches, _ = sh.skeleton(g)
    nr, br = roots(nodes, branches, N)
    assert len(nodes) and len(branches) and not (nr & br)
    assert (N ** 3) % 64 and len({p >> 6 for p in nr} & {p >> 6 for p in br}) >= 2      # words with roots of both kinds
    assert 63 in nr and 64 in br and 65 in nr                                            # the run 63, 64, 65 crosses the first boundary
    flat = labels.reshape(-1)
    assert flat[63] and not flat[63] & BRANCH and flat[64] & BRANCH and flat[65] and not flat[65] & BRANCH
    assert (nodes["voxels"] == 1).all() and (branches["voxels"] == 1).all()              # every root is a voxel of its own
    _, table = ch.components(g, 0, 26)
    assert len(table) == len(nodes) - len(branches)                                      # a bar's three roots are one root of a component
    assert 63 in {int(f) for f in table["first"]} and set(table["voxels"].tolist()) == {1, 3}


@pytest.mark.gpu
@pytest.mark.parametrize("N", (6, 10))
def test_both_numberings_equal_the_host_routines_on_the_pattern(dxvlib, bunny, N):
    import dxrvoxelizer_amd
    vb, ib, _ = bunny
    g = pattern(N)
    v = dxrvoxelizer_amd.Voxelizer(0)
    try:
        v.InitFromArrays(vb, ib)
        v.Voxelize(N)
        write_grid(v, g)
        labels, nodes, branches = v.Skeleton()
        want = sh.skeleton(g)
        assert labels.tobytes() == want[0].tobytes() and nodes.tobytes() == want[1].tobytes() and branches.tobytes() == want[2].tobytes()
        info = v.SkeletonInfo()
        assert (info["nodes"], info["branches"], info["end_voxels"], info["curve_voxels"], info["junction_voxels"]) == (len(nodes), len(branches)) + want[3]
        labels, table = v.Components(dxrvoxelizer_amd.COMP_SOLID, 26)
        wantLabels, wantTable = ch.components(g, 0, 26)
        assert labels.tobytes() == wantLabels.tobytes() and table.tobytes() == wantTable.tobytes()
    finally:
        v.close()
