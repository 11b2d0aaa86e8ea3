"""The LBVH build rule on the CPU: the numpy restatement (tests/lbvh_restated.py, written from the comments) against the product's own
headers compiled for the host (tests/hostcheck: morton_key, karras_node, tri_box, compress_node, widen_node), on every family of
tests/lbvh_meshes.py but the two 2 M-triangle cases.  This is where karras_node meets a reference that is not itself: keys, links,
both child boxes, both child heights and the root's height, word for word.  Each family's own condition -- what makes it reach its
branch -- is asserted on the restatement's side."""
import ctypes as C

import numpy as np
import pytest

import lbvh_meshes as lm
import lbvh_restated as lr


@pytest.fixture(scope="module")
def builds():
    cache = {}

    def get(name):
        if name not in cache:
            cache[name] = lr.Build(*lm.get(name))
        return cache[name]
    return get


@pytest.mark.parametrize("name", lm.NAMES)
def test_restated_build_equals_host_code(hostcheck, builds, name):
    vb, ib = lm.get(name)
    r = builds(name)
    h = hostcheck(vb, ib, r.bound)
    assert np.array_equal(r.keys, h.keys()), "Morton keys differ"
    assert r.height == h.height, "root height differs"
    want = h.nodes()
    if r.T == 1:
        assert np.array_equal(want[0, :3].view(np.float32), r.lo[0]) and np.array_equal(want[0, 3:6].view(np.float32), r.hi[0])
        return
    assert np.array_equal(r.nodes[:, 12:14], want[:, 12:14]), "hierarchy differs from the radix tree"
    assert np.array_equal(r.nodes[:, 14:16], want[:, 14:16]), "child heights differ"
    assert np.array_equal(r.nodes[:, :12], want[:, :12]), "child boxes differ"
    # the tree is a tree: every node but the root and every leaf has one parent word, and it points back
    p = r.parents
    kids = r.links[p[1:] >> 1, p[1:] & 1]
    slots = np.arange(1, 2 * r.T - 1)
    assert np.array_equal(kids, np.where(slots < r.T - 1, slots, ~(slots - (r.T - 1))))
    # the host code's half-float copies hold the properties the device's downloads are held to
    assert len(lr.outward_violations(want, h.nodes32())) == 0
    assert np.array_equal(lr.wide_from_32(h.nodes32()), h.nodes64())


def run_lengths(keys):
    code = keys >> np.uint64(32)
    edges = np.flatnonzero(np.concatenate([[True], code[1:] != code[:-1], [True]]))
    return np.diff(edges)


def test_runs_has_long_runs_of_equal_codes_with_scattered_indices(builds):
    r = builds("runs")
    runs = run_lengths(r.keys)
    assert runs.max() >= 257 and (runs > 1).sum() >= 100 and (runs == 1).sum() >= 100
    assert set(np.unique(runs)) >= set(lm.RUN_LENGTHS)
    assert 2500 <= r.T <= 3500 and 200 <= len(runs) <= 600
    start = int(np.flatnonzero(np.concatenate([[True], (r.keys >> np.uint64(32))[1:] != (r.keys >> np.uint64(32))[:-1]]))[np.argmax(runs)])
    idx = r.order[start:start + runs.max()]
    assert (np.diff(idx) > 1).sum() > runs.max() // 2, "the longest run's triangle indices are consecutive"


@pytest.mark.parametrize("T", lm.COPIES)
def test_copies_is_one_run(builds, T):
    r = builds(f"copies-{T}")
    assert run_lengths(r.keys).tolist() == [T]


@pytest.mark.parametrize("b", lm.COMB_BITS)
def test_comb_height_is_31_plus_b(builds, b):
    r = builds(f"comb-{b}")
    assert r.T == (1 << b) + 1
    assert r.height == 31 + b
    code = np.unique(r.keys >> np.uint64(32))
    full = (1 << 30) - 1
    assert set(full ^ ((1 << (30 - k)) - 1) for k in range(31)) <= set(int(c) for c in code)
    assert run_lengths(r.keys)[-1] == 2 + b


def test_comb_soup_is_as_high_as_the_comb_and_its_walk_is_deep(hostcheck, builds):
    """height 39 like comb-8, and rays that hold more entries than an 8-entry column has: the host's walk, per ray, at 16^3"""
    r = builds("comb-8-soup")
    assert r.height == 39 and builds("comb-8").height == 39
    vb, ib = lm.get("comb-8-soup")
    h = hostcheck(vb, ib, r.bound)
    out, hist = np.zeros(8, np.uint64), np.zeros(64, np.uint64)
    hostcheck.lib.hc_trace_stats.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p]
    hostcheck.lib.hc_trace_stats(h.h, 16, 1, out.ctypes.data_as(C.c_void_p), hist.ctypes.data_as(C.c_void_p))
    assert out[0] == 4096 and out[3] > 8 and hist[9:].sum() > 0
    for name, deepest in (("comb-7", 2), ("comb-8", 3)):                       # the combs themselves: a high tree, a shallow walk
        vb, ib = lm.get(name)
        h = hostcheck(vb, ib, builds(name).bound)            # (named: the scene lives as long as the object does)
        hostcheck.lib.hc_trace_stats(h.h, 16, 1, out.ctypes.data_as(C.c_void_p), hist.ctypes.data_as(C.c_void_p))
        assert out[0] == 4096 and out[3] == deepest


@pytest.mark.parametrize("axis", range(3))
def test_flat_has_one_cell_coordinate(builds, axis):
    r = builds(f"flat-{'xyz'[axis]}")
    q = lr.cells(r.lo, r.hi)
    assert len(np.unique(q[:, axis])) == 1
    assert all(len(np.unique(q[:, a])) > 100 for a in range(3) if a != axis)
    assert np.all(r.hi[:, axis] - r.lo[:, axis] == 2 * lr.PAD)


def test_clamped_reaches_both_clamps_on_every_axis(builds):
    r = builds("clamped")
    assert np.array_equal(r.bound, np.array([0, 0, 0, 1], np.float32))
    q = lr.cells(r.lo, r.hi)
    centre = (r.lo + r.hi) * np.float32(0.5)
    for axis in range(3):
        assert (q[:, axis] == 0).any() and (q[:, axis] == 1023).any()
        assert (centre[:, axis] == -1).any(), "no centre on the lower clamp"                       # u = 0: not above 0
        assert ((centre[:, axis] * np.float32(0.5) + np.float32(0.5)) * np.float32(1024) > 1023).any(), "no centre above the upper clamp"


def test_giant_and_tiny_mixes_boxes_of_the_bound_with_boxes_of_the_pad(builds):
    r = builds("giant-and-tiny")
    size = (r.hi - r.lo).max(1)
    assert (size > 1.9).sum() == 3 and (size < 2 * lr.PAD + 1e-6).sum() == 2000


def test_counts_reach_the_sampling_and_pyramid_branches(builds):
    """the arithmetic that picks the cases: workgroups of 256 and the key sampling stride, pyramid slots of 1024 * 2^k"""
    def groups(T):
        return (T + 255) // 256
    assert groups(65536) == 256 and groups(65537) == 257 and groups(65537) // 256 == 1
    assert groups(131073) == 513 and groups(131073) // 256 == 2 and 131073 - 512 * 256 == 1 and 512 % 2 == 0   # the last sampled group holds one triangle
    assert groups(65793) == 258 and groups(65793) // 256 == 1 and 65793 - 257 * 256 == 1                 # stride 1, a last group of one triangle
    for T, slots in ((1024, 1024), (1025, 2048), (2048, 2048), (2049, 4096)):
        P = 1024
        while P < T:
            P *= 2
        assert P == slots
    for T in (65793, 131073):
        r = builds(f"count-{T}")
        every = (r.hi[:, 1] - r.lo[:, 1]) + (r.hi[:, 2] - r.lo[:, 2])
        assert r.tri_extent > 0 and abs(float(r.tri_extent) - float(every.mean()) / 2) < 0.01 * float(r.tri_extent)
