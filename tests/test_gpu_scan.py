"""The exclusive scan under the grid operators (csrc/scan.hip, csrc/dxv_scan.h) on its own, through the test hook dxv_debug_scan, against
numpy's cumulative sum in uint64.  what = 0 is launch_scan_words -- block sums, the scan of the sums, the add-back, as octree, components and
isosurface call it --, what = 1 launch_scan_sums alone with the totals right behind the sums, as thickness and partition call it.

The sizes are the ones at which the code takes another path: one word, less than a wave, one word less than / exactly / one word more than a
block of 1024, several blocks with a ragged end, and 1024 * 1024 + 5 words = 1025 block sums, where a thread of the one workgroup that scans
the sums takes TWO of them (chunk = 2), thread 512 takes the one that is left and threads 513 .. 1023 an empty, clamped range.  Of the
operator tests that path (more than 2^20 words, or a grid side of 102 for thickness and partition) is reached by test_gpu_thickness_sides.py at
126, 130 and 194, by test_gpu_access_sides.py at the same sides out of access's own scratch layout, by test_gpu_partition_sides.py at 102,
126, 130 and 194 -- there also under the heads' scan, with more than 2^20 interface faces -- and by test_gpu_flood_wide_rounds.py at 160 and
162 through the intrusion map."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

WORDS = [1, 63, 1023, 1024, 1025, 4099, 1024 * 1024 + 5]
BLOCKS = [1, 364, 1024, 1025, 2049, 5000]
GUARD = 0xA5A5A5A5A5A5A5A5


@pytest.fixture(scope="module")
def v(dxvlib):
    import dxrvoxelizer_amd
    w = dxrvoxelizer_amd.Voxelizer(0)
    try:
        yield w
    finally:
        w.close()


def counts(kind, words, lanes):
    rng = np.random.default_rng(words * 8 + lanes)
    if kind == "zero":
        return np.zeros((words, lanes), np.uint32)
    if kind == "sparse":                                                # what the operators produce: popcounts of words that are mostly empty
        return (rng.integers(0, 65, (words, lanes)) * (rng.random((words, lanes)) < 0.2)).astype(np.uint32)
    return rng.integers(0, 1 << 32, (words, lanes), dtype=np.uint64).astype(np.uint32)      # full range: block sums and totals pass 2^32, the stored prefix wraps


def exclusive(a):
    wide = a.astype(np.uint64)
    return np.cumsum(wide, axis=0, dtype=np.uint64) - wide, wide.sum(axis=0, dtype=np.uint64)


def check_words(v, kind, words, lanes):
    a = counts(kind, words, lanes)
    want, totals = exclusive(a)
    got = a.copy()
    assert v.debug_scan(0, lanes, got, words) == [int(t) for t in totals], (kind, words, lanes)
    assert np.array_equal(got, (want & np.uint64(0xFFFFFFFF)).astype(np.uint32)), (kind, words, lanes, np.flatnonzero((got != want.astype(np.uint32)).any(axis=1))[:4])


@pytest.mark.parametrize("lanes", [1, 2])
@pytest.mark.parametrize("words", WORDS)
@pytest.mark.parametrize("kind", ["sparse", "zero"])
def test_the_prefix_of_every_word_and_the_totals(v, kind, words, lanes):
    check_words(v, kind, words, lanes)


@pytest.mark.parametrize("lanes", [1, 2])
def test_full_range_counts_wrap_the_prefix_and_not_the_totals(v, lanes):
    words = WORDS[-1]
    assert int(exclusive(counts("full", words, lanes))[1].min()) > 1 << 32
    check_words(v, "full", words, lanes)


@pytest.mark.parametrize("lanes", [1, 2])
@pytest.mark.parametrize("blocks", BLOCKS)
def test_the_scan_of_block_sums_with_the_totals_behind_them(v, blocks, lanes):
    rng = np.random.default_rng(blocks * 8 + lanes)
    sums = rng.integers(0, (1 << 40) + 1, (blocks, lanes), dtype=np.uint64)
    want, totals = exclusive(sums)
    buf = np.concatenate([sums.ravel(), np.full(lanes + 1, GUARD, np.uint64)])     # the sums, room for the totals, one word nothing may write
    assert v.debug_scan(1, lanes, buf, blocks) == [int(t) for t in totals]
    assert np.array_equal(buf[: blocks * lanes].reshape(blocks, lanes), want), (blocks, lanes)
    assert np.array_equal(buf[blocks * lanes: (blocks + 1) * lanes], totals) and int(buf[-1]) == GUARD


@pytest.mark.parametrize("what", [0, 1])
@pytest.mark.parametrize("lanes,items,null", [(0, 70, False), (3, 70, False), (1, 0, False), (2, 0, False), (1, 70, True), (2, 70, True)])
def test_what_the_entry_points_refuse_is_an_error_and_leaves_the_buffer_alone(v, what, lanes, items, null):
    import dxrvoxelizer_amd
    buf = np.arange(1, 4 * 71 + 2, dtype=np.uint32 if what == 0 else np.uint64)       # (room for any of the cases)
    before = buf.copy()
    with pytest.raises(dxrvoxelizer_amd.DxvError, match="dxv_debug_scan failed: invalid argument"):
        v.debug_scan(what, lanes, None if null else buf, items)
    assert np.array_equal(buf, before)
    check_words(v, "sparse", 1025, 2)                                   # (and the context goes on)
