"""The lists' start table (dxv_dirmap.h: dm_start_word, dm_start_offset) on the CPU, through tests/hostcheck/start_table_check.cpp.

For every texel and every probe radius -- each entry's far radius and the halfs next to it, the half below the first entry's, r1max -- the
table's start lies at or in front of the exact first entry with !(r1 < near) and at or behind the first entry of the ray's bucket rounded
down by the table's unit; and grids through the kernels' own bodies are the same with the table as without it."""
import ctypes as C

import numpy as np
import pytest

from start_table_cases import HostLists, library, made_up_lists, stack, two_shells


def check_probe(p, what):
    print(what, p)
    assert p["probes"] > 0 and p["late"] == 0 and p["early"] == 0, (what, p)


@pytest.mark.parametrize("name,R", [("bunny", 64), ("bunny", 256), ("dragon", 64), ("dragon", 256)])
def test_meshes_every_texel_every_probe(request, name, R):
    vb, ib, _ = request.getfixturevalue(name)
    h = HostLists(vb, ib, R)
    try:
        p = h.probe()
        check_probe(p, (name, R))
        assert p["moved"] > 0                                          # (the table does say something on a real mesh)
    finally:
        h.close()


def test_two_shells_and_the_stack():
    h = HostLists(*two_shells(), 64)
    try:
        p = h.probe()
        check_probe(p, "two shells")
        assert p["moved"] > p["probes"] // 8                           # rays between and behind the shells skip the near one
        for N in (32, 50):
            assert np.array_equal(h.voxelize(N, True), h.voxelize(N, False)), N
        g1, t1 = h.voxelize(32, True, texels=True)
        g0, t0 = h.voxelize(32, False, texels=True)
        assert np.array_equal(g1, g0) and np.array_equal(t1, t0) and g0.any()
    finally:
        h.close()
    h = HostLists(*stack(300), 16)
    try:
        p = h.probe()
        check_probe(p, "stack of 300")
        assert p["over_255"] >= 1 and p["longest"] >= 300               # one texel counts in units of two
        a, b = h.voxelize(32, True), h.voxelize(32, False)
        assert np.array_equal(a, b) and a.any()
    finally:
        h.close()


def test_bunny_grids_with_and_without_the_table(bunny):
    vb, ib, _ = bunny
    h = HostLists(vb, ib, 64)
    try:
        for N in (64, 50):
            g = h.voxelize(N, False)
            assert np.array_equal(h.voxelize(N, True), g) and g.any(), N
    finally:
        h.close()


def test_made_up_lists():
    """lists of 1, 8 and 9 entries, lists whose far radii are all equal (top - k0 = 0), two shells in 9 .. 35 entries, a list over the whole
    range of halfs (the largest shift), lists of 255 .. 257, 511 .. 513 and 65,535 entries (units of 1, 2, 3 and 256)"""
    L = library()
    rng = np.random.default_rng(7)
    lists = [[], [0x3800], [0x0400], [0x7bff]]
    lists += [sorted(rng.integers(0x3000, 0x3a00, n).tolist()) for n in (8, 9, 9, 17, 18, 35, 36)]
    lists += [[0x3456] * n for n in (1, 8, 9, 40, 300)]
    lists += [sorted([0x3400 + int(x) for x in rng.integers(0, 6, n // 2)] + [0x3900 + int(x) for x in rng.integers(0, 6, n - n // 2)]) for n in (9, 12, 17, 25, 35)]
    lists += [sorted(rng.integers(0x0400, 0x7c00, 64).tolist()), [0x0400, 0x7bff], [0x0400] * 5 + [0x7bff]]
    lists += [sorted(rng.integers(0x2000, 0x4000, n).tolist()) for n in (255, 256, 257, 511, 512, 513, 65535)]
    lists += [[0x3000] * 400 + [0x3800] * 200, [0x3000 + k // 3 for k in range(700)]]
    cells, entries = made_up_lists(lists)
    starts = np.zeros(len(cells), np.uint32)
    out = np.zeros(8, np.uint64)
    L.st_probe_raw(cells.ctypes.data_as(C.c_void_p), len(cells), entries.ctypes.data_as(C.c_void_p), starts, out.ctypes.data_as(C.c_void_p))
    p = dict(zip(("probes", "late", "early", "texels", "over_255", "longest", "moved", "first_bad"), (int(x) for x in out)))
    check_probe(p, "made-up lists")
    assert p["texels"] == len(lists) - 1 and p["longest"] == 65535 and p["moved"] > 0
    assert starts[0] == 0 and starts[1] == 0                            # no entries, one entry: nothing to skip
    # all far radii equal: shift 0 and no entry in any bucket but the last
    for k, keys in enumerate(lists):
        if len(set(keys)) == 1:
            assert starts[k] == 0, (k, hex(starts[k]))
    # two shells of 9 entries: a ray that starts between them skips the near shell exactly
    k = next(i for i, keys in enumerate(lists) if len(keys) == 9 and keys[-1] >= 0x3900 and keys[0] < 0x3410)
    near_shell = sum(1 for x in lists[k] if x < 0x3800)
    near = np.frombuffer(np.array([0x3880], np.uint16).tobytes(), np.float16)[0]
    assert L.st_offset(int(starts[k]), 9, lists[k][-1], float(near)) == near_shell
    # a ray beyond r1max, and one in front of every entry, skip nothing
    assert L.st_offset(int(starts[k]), 9, lists[k][-1], 60000.0) == 0 and L.st_offset(int(starts[k]), 9, lists[k][-1], 1e-3) == 0
