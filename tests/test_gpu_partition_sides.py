"""Every even side from 2 to 72, four longer rows, and four grids with many regions and faces, through dxv_partition on the GPU for both kinds at
cap_sq 10 (tests/grid_sides.py: the sides, the grids and why these).  The header's routines are run on the CPU by tests/test_partition_rule.py;
what exists only in partition.hip -- the wave per brick with its partial bricks at N % 4 = 2, the mips' wave maxima, the blocks' scans, the
wave-wide stats, the sort and the atomics of the throats -- runs here.  Each grid is written through the frame's grid pointer; labels, table and
throats are compared as bytes with the numpy restatement (form (a)) to side 72 and with the host library (tests/partition_host.py) above, at
102 with both.
  102, 126, 130, 194   more than 1024 block sums under k_part_count / k_part_number (N >= 102: chunk 2 of the scan), rows of two to four words.
  the wide cases       "random 0.3" where the sweep's largest region count, 39114 at side 72, stops short:
      102 solid        K = 110021: labels of 17 bits, a pair of labels of 34, a sort of 4 passes
      130 empty        1052426 interface faces: more than 2^20 under the heads' scan (k_part_count_heads, k_part_emit_pairs)
      194 empty        3521131 faces: the sort leaves its small shape (more than 2 * 2^20 keys); K = 255887, pairs of 36 bits
      194 solid        K = 756495: labels of 20 bits, pairs of 40; once more without throats
Each wide case asserts its condition on the expectation before it compares.  The host library takes 0.03 .. 0.5 s per call at 102, 1.3 s at the
most at 126 and 130, 0.3 .. 4.9 s at 194 (an item there: 4.3 s "all 0xFF", 5.2 s "ends"); the wide cases 1.1, 0.7, 2.3 and 1.2 s; the
restatement 1.3 and 1.5 s for the two kinds of "random 0.3" at 102."""
import pytest

import grid_sides as gs
import partition_host as ph
import partition_restated as pr
from raycast_restated import write_grid

pytestmark = pytest.mark.gpu
CAP = 10
LONGER = ([(102, name) for name in ("random 0.6", "random 0.3", "all 0xFF", "hollow box", "ends")] +      # 102 takes the sweep's five grids,
          [(N, name) for N in gs.WIDE for name in ("all 0xFF", "ends")])                                   # the others the two of the other sweeps
WHAT = ("labels", "table", "throats")
# (side, kind, what the expectation must show for the case to reach what it is there for)
WIDE_CASES = {"102 solid: 17-bit labels": (102, pr.SOLID, lambda table, throats: len(table) >= 65536),
              "130 empty: more than 2^20 faces": (130, pr.EMPTY, lambda table, throats: int(throats["faces"].sum()) > 2 ** 20),
              "194 empty: more than 2 * 2^20 faces": (194, pr.EMPTY, lambda table, throats: int(throats["faces"].sum()) > 2 * 2 ** 20),
              "194 solid: 20-bit labels": (194, pr.SOLID, lambda table, throats: len(table) >= 2 ** 19)}


@pytest.fixture(scope="module")
def writer(dxvlib, bunny):
    """the one Voxelizer, on the bunny, whose frame every grid of this file is written into"""
    import dxrvoxelizer_amd
    vb, ib, _ = bunny
    v = dxrvoxelizer_amd.Voxelizer(0)
    v.InitFromArrays(vb, ib)
    yield v
    v.close()


def check_both_kinds(v, N, name, g):
    """labels, table and throats of both kinds of the selected frame's grid, which holds g, against the restatement"""
    for of in (pr.SOLID, pr.EMPTY):
        want = pr.partition(g, of, CAP)
        got = v.Partition(of, CAP)
        for a, b, what in zip(got, want, WHAT):
            assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes(), (N, name, of, what)


def check_against_the_host_library(v, N, name, g, of, want=None):
    """labels, table, throats and the counts of one kind of the selected frame's grid, which holds g; returns the expectation"""
    if want is None:
        want = ph.partition(g, of, CAP)
    got = v.Partition(of, CAP)
    for a, b, what in zip(got, want, WHAT):
        assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes(), (N, name, of, what)
    assert v.PartitionInfo()[1:] == (len(want[1]), len(want[2]), want[3][0]), (N, name, of)
    return want


@pytest.mark.parametrize("N", gs.SWEEP)
def test_both_kinds_at_every_side(writer, N):
    v = writer
    v.Voxelize(N)
    seen = 0
    for name, g in gs.grids(N):
        seen += 1
        write_grid(v, g)
        check_both_kinds(v, N, name, g)
    assert seen == (5 if N >= 6 else 4)


@pytest.mark.parametrize("N, name", LONGER)
def test_both_kinds_at_the_longer_rows(writer, N, name):
    v = writer
    if v.stats()["grid_dim"] != N:
        v.Voxelize(N)
    g = dict(gs.grids(N, (name,)))[name]
    write_grid(v, g)
    for of in (pr.SOLID, pr.EMPTY):
        want = check_against_the_host_library(v, N, name, g, of)
        if (N, name) == (102, "random 0.3"):
            for a, b, what in zip(want, pr.partition(g, of, CAP), WHAT):
                assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes(), (N, name, of, what, "host library against the restatement")


@pytest.mark.parametrize("case", list(WIDE_CASES))
def test_many_regions_and_many_faces(writer, case):
    N, of, reaches = WIDE_CASES[case]
    v = writer
    if v.stats()["grid_dim"] != N:
        v.Voxelize(N)
    g = dict(gs.grids(N, ("random 0.3",)))["random 0.3"]
    write_grid(v, g)
    want = ph.partition(g, of, CAP)
    assert reaches(want[1], want[2]), (case, len(want[1]), int(want[2]["faces"].sum()))
    assert int(want[2]["faces"].sum()) == want[3][0]
    check_against_the_host_library(v, N, "random 0.3", g, of, want)
    if case != "194 solid: 20-bit labels":
        return
    import dxrvoxelizer_amd as dxv                                      # without throats: the same labels, the same table but for its throat counts, no throats
    labels, table, throats = v.Partition(of, CAP, throats=False)
    stripped = want[1].copy()
    stripped["throats"] = 0
    assert throats is None and labels.tobytes() == want[0].tobytes() and table.tobytes() == stripped.tobytes() and want[1]["throats"].any()
    assert v.PartitionInfo()[1:] == (len(table), 0, 0)
    with pytest.raises(dxv.DxvError, match="made without throats"):
        v.PartitionThroats()
