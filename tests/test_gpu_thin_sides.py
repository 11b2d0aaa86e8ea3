"""Every even side from 2 to 72, and three longer rows, through dxv_thin on the GPU for both kinds, unbounded and stopped after two iterations, in
batches of the default size and with every iteration settled on the host (tests/grid_sides.py: the sides, the grids and why these).  The
header's routines are run at the same sides on the CPU by tests/test_thin_rule.py; what exists only in thin.hip and in the morph's pack and
write-back -- the neighbour-word guards of k_thin_border, k_thin_sub's lane -> (word, row) mapping with half = N >> 1, the prev / next words
of the nine row triples, the partial last block, the in-place store, the guarded byte path with loose bytes at N % 8 != 0, the batches' control
block -- runs here.  Each grid is written through the frame's grid pointer; grid bytes, CountSolid and thin_info's iterations, removed count
and verdict are compared (test_gpu_thin.check_thin).  The expectation is the numpy restatement for every grid to side 32, for "all 0xFF",
"ends" and "hollow box" at every side and for "random 0.3" to 72; for "random 0.6" above 32 it is the host library through its byte path,
which the rule test holds to the restatement at the same sides' other grids and at 66 (the restatement of that grid takes 6 s at 72).  At the
longer rows "all 0xFF" takes 64, 66 and 98 iterations: more than one batch even at thinrounds 64.  A last test thins at 194 and then goes
down through 70, 66, 38, 6 and 2 on the same Voxelizer: the thin in the scratch a larger grid left behind (DevBuf::reserve keeps an allocation
that is large enough), with bits set behind a row's end and rows of another word count in memory."""
import pytest

import grid_sides as gs
import thin_host
import thin_restated as tr
from raycast_restated import write_grid
from test_gpu_thin import check_thin

pytestmark = pytest.mark.gpu

LIMITS = (0, 2)
LOSING = ("all 0xFF", "random 0.6", "random 0.3")                      # the grids every side must take voxels from where the kernels' guards sit
DESCENT = (70, 66, 38, 6, 2)                                            # after 194: same word count as 72 with other bits behind the end; one word after two; the smallest
DESCENT_GRIDS = ("random 0.3", "ends")

_WANT = {}


@pytest.fixture(scope="module")
def writer(dxvlib, bunny):
    """the one Voxelizer, on the bunny, whose frame every grid of this file is written into"""
    import dxrvoxelizer_amd
    vb, ib, _ = bunny
    v = dxrvoxelizer_amd.Voxelizer(0)
    v.InitFromArrays(vb, ib)
    yield v
    v.close()


def names_at(N):
    """the grids of a side: the sweep's five (four below 6), three of them at the longer rows"""
    return gs.WIDE_GRIDS if N in gs.WIDE else None


def compute(N, name, g, kind, limit):
    if name == "random 0.6" and N > 32:
        return thin_host.thin(g, kind, limit, eight_at_once=False)
    assert N <= 32 or name in ("all 0xFF", "ends", "hollow box") or (name == "random 0.3" and N <= 72), (N, name)
    return tr.thin(g, kind, limit)


def expectation(N, name, g, kind, limit):
    """(grid, iterations, removed, converged), made once per (grid, kind, limit); the ones the descent needs again are kept, unchanged"""
    key = (N, name, kind, limit)
    if key in _WANT:
        return _WANT[key]
    want = compute(N, name, g, kind, limit)
    if N in DESCENT and name in DESCENT_GRIDS and limit == 0:
        want[0].setflags(write=False)
        _WANT[key] = want
    return want


def assert_not_empty(N, name, g, kind, want):
    """on the expectation alone: an unbounded thin takes voxels on both sides of a row's first word boundary, at the row's last bit, in the last
    row of a slice and in the last slice -- where a guard of the kernels decides.  (Checked with the host library at every side of the sweep:
    hundreds of voxels each above 64; the last row and the last slice lose voxels in all three grids from side 6 on -- at 2 and 4 "random 0.3"
    holds a handful of voxels and CURVE takes none of the last slice.)  Nothing of the kind is claimed for "ends": under CURVE it is a fixed point
    at several sides, a legitimate case."""
    grid, iterations, removed, converged = want
    assert converged, (N, name, kind)
    went = (g != 0) & (grid == 0)
    if name in LOSING:
        if N > 64:
            for x in (63, 64, N - 1):
                assert went[:, :, x].any(), (N, name, kind, x)
        if N >= 6:
            assert went[:, N - 1, :].any() and went[N - 1].any(), (N, name, kind)
    if name == "all 0xFF" and N in gs.WIDE:                             # a layer per iteration and one that finds nothing: 64 at 126, a full batch; 66 and 98, more than one
        assert iterations == N // 2 + 1 and (iterations > 64 or N == 126), (N, kind, iterations)


def thin_both_batch_sizes(v, N, name, g, kind, limit, want, batches):
    try:
        for rounds in batches:
            v.set_option("thinrounds", rounds)
            check_thin(v, g, lambda: write_grid(v, g), kind, want, f"N = {N}, {name}, thinrounds {rounds}", limit=limit)
    finally:
        v.set_option("thinrounds", 0)


@pytest.mark.parametrize("N", gs.SWEEP + gs.WIDE)
def test_both_kinds_at_every_side(writer, N):
    v = writer
    v.Voxelize(N)
    batches = (0, 64) if N in gs.WIDE else (0, 1)                       # thinrounds 1: every iteration is settled on the host
    seen, full = 0, None
    for name, g in gs.grids(N, names_at(N)):
        seen += 1
        for kind in tr.KINDS:
            for limit in LIMITS:
                want = expectation(N, name, g, kind, limit)
                if limit == 0:
                    assert_not_empty(N, name, g, kind, want)
                if (name, kind, limit) == ("all 0xFF", tr.KERNEL, 0):
                    full = want
                thin_both_batch_sizes(v, N, name, g, kind, limit, want, batches)
    assert seen == (3 if N in gs.WIDE else 5 if N >= 6 else 4)
    assert int(full[0].sum()) == 1 and full[2] == N ** 3 - 1            # an all-solid grid thins from its border, down to one voxel


def test_smaller_sides_in_the_scratch_of_a_larger_one(writer):
    """194, then 70, 66, 38, 6 and 2 on the same Voxelizer: masks, border, loose bits and control block lie in what the four-word rows of 194 left"""
    v = writer
    N = gs.WIDE[-1]
    v.Voxelize(N)
    (name, g), = gs.grids(N, ("all 0xFF",))
    for kind in tr.KINDS:                                               # two iterations of the full grid leave every mask of the scratch full of bits
        check_thin(v, g, lambda: write_grid(v, g), kind, tr.thin(g, kind, 2), f"N = {N}, {name}", limit=2)
    for N in DESCENT:
        v.Voxelize(N)
        seen = 0
        for name, g in gs.grids(N, DESCENT_GRIDS):
            seen += 1
            for kind in tr.KINDS:
                want = expectation(N, name, g, kind, 0)
                if N > 64:
                    assert_not_empty(N, name, g, kind, want)
                check_thin(v, g, lambda: write_grid(v, g), kind, want, f"N = {N} after 194, {name}")
        assert seen == 2
