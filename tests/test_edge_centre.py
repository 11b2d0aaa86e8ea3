"""The lists' edge word with cells counted from the texel's centre (dxv_dirmap.h: dm_ray_local, dm_local_entry), on the CPU through the
product's own __host__ __device__ code (tests/hostcheck/filter_check.cpp):

  1  the byte test is conservative: wherever the real-valued dilated edge function of the stored edge (double, the record's own pad) is
     >= 0 anywhere in a cell, the edge term of dm_local_pass passes in that cell -- every one of the 128 x 128 cells of a few thousand
     (record, texel) pairs, zero exceptions;
  2  the lists path gives the oracle's grids bit for bit: the turned octahedron, its lattice-snapped version and the golden bunny at 16^3,
     32^3 and 64^3 on maps of 16, 64 and 256 texels;
  3  the replay of the lists kernel's loop on the headline workload (torus1m, 512^3, 512 texels, every 32nd brick layer) keeps the bounds the
     parent's measured values set: triangle tests per brick <= 74.0 (parent 77.5), triangle rounds <= 2.70 (parent 2.81), scan rounds within
     0.02 of the parent's 2.37, and exactly the parent's tests that hit -- a filter may drop only tests that find nothing."""
import ctypes as C

import numpy as np
import pytest

import edge_centre_cases as cases
from tools.filter_stats import library, replay


@pytest.fixture(scope="module")
def lib():
    return library()


def test_byte_test_is_conservative(lib):
    recs = cases.records(np.random.default_rng(20261020))
    assert len(recs) >= 3000
    passes, real, emax = np.zeros(128 * 128, np.uint8), np.zeros(128 * 128, np.uint8), np.zeros(3 * 128 * 128, np.float64)
    which = C.c_int32(0)
    bad, seen = [], {}
    with_edge = identified = cutting = clamped_low = at_limit = diagonal = 0
    for what, R, i, j, rec in recs:
        edge = lib.fc_edge_cells(rec.ctypes.data_as(C.c_void_p), R, i, j, passes, real, emax, C.byref(which))
        kind = what.split(" ")[0]
        seen[kind] = seen.get(kind, 0) + 1
        if edge == 0:
            if not passes.all():
                bad.append((what, R, i, j, "no edge, yet a cell fails"))
            continue
        with_edge += 1
        a, b, c1, c2 = (int(x) for x in np.array([edge], np.uint32).view(np.int8))
        c = 127 * c1 + c2
        diagonal += abs(a) == 127 and abs(b) == 127
        clamped_low += c == -16256
        at_limit += abs(c) >= 16000
        cutting += not passes.all()
        if which.value >= 0:
            identified += 1
            must = emax[which.value * 16384:(which.value + 1) * 16384] >= 0.0
        else:
            must = real != 0                                # (the stored edge not told apart: at least where every edge function is reached)
        wrong = must & (passes == 0)
        if wrong.any():
            at = int(np.flatnonzero(wrong)[0])
            bad.append((what, R, i, j, hex(edge), "edge %d" % which.value, "cell (%d, %d)" % (at % 128, at // 128), int(wrong.sum())))
    print("records", len(recs), seen, "with an edge", with_edge, "identified", identified, "cutting", cutting, "diagonal", diagonal,
          "c near a limit", at_limit, "c clamped low", clamped_low)
    assert not bad, (len(bad), bad[:20])
    # the cases are what they claim to be: most records store an edge that cuts cells off, the 45-degree normals and the clamp are met
    assert with_edge >= len(recs) // 2 and identified >= with_edge * 9 // 10 and cutting >= with_edge // 2
    assert diagonal >= 100 and at_limit >= 20 and clamped_low >= 1


@pytest.fixture(scope="module")
def wanted(orc, bunny):
    """(vb, ib, {N: the oracle's grid}) per mesh: computed once, never written to"""
    out = {}
    for name, (vb, ib) in cases.meshes(bunny).items():
        scene = orc.Scene(vb, ib)
        out[name] = (vb, ib, {N: scene.voxelize(N) for N in (16, 32, 64)})
    return out


@pytest.mark.parametrize("R", (16, 64, 256))
@pytest.mark.parametrize("name", ("octahedron", "snapped", "bunny"))
def test_host_lists_path_gives_the_oracles_grid(lib, orc, wanted, name, R):
    vb, ib, want = wanted[name]
    vb, ib = np.ascontiguousarray(vb, np.float32), np.ascontiguousarray(ib, np.uint32)
    _, b = orc.bound(vb)
    h = lib.hc_scene_create(vb, len(vb), ib, len(ib) // 3, b)
    try:
        n = lib.hc_dirmap_build(h, R)
        assert 0 < n < 2 ** 63
        starts = np.zeros(6 * R * R, np.uint32)
        lib.st_table(h, starts)
        census = np.zeros(2, np.uint64)
        lib.fc_edge_census(h, census)
        print(name, R, "entries", int(census[0]), "without an edge", int(census[1]))
        assert census[0] == n and (name == "bunny" and R == 16 or census[1] < census[0])      # (the edge word is in play)
        for N, grid in want.items():
            for table in (None, starts.ctypes.data_as(C.c_void_p)):
                got = np.zeros((N, N, N), np.uint8)
                assert lib.st_voxelize(h, N, 2, table, got, None) == 0
                assert np.array_equal(got, grid), (name, R, N, table is not None, int((got != grid).sum()))
    finally:
        lib.hc_scene_destroy(h)


def test_replay_keeps_the_bounds_of_the_parents_measurement(lib, orc):
    from bench import make_mesh
    vb, ib, _ = make_mesh("torus1m")
    vb, ib = np.ascontiguousarray(vb, np.float32), np.ascontiguousarray(ib, np.uint32)
    _, b = orc.bound(vb)
    h = lib.hc_scene_create(vb, len(vb), ib, len(ib) // 3, b)
    try:
        res = replay(lib, h, 512, 512, 32)
    finally:
        lib.hc_scene_destroy(h)
    got, floor = res["shipped"], res["perfect_filter"]
    per = got["per_brick"]
    print(res)
    assert got["bricks"] == 12544
    assert per["triangle_tests"] <= 74.0
    assert per["triangle_rounds"] <= 2.70
    assert abs(per["scan_rounds"] - 2.37) <= 0.02
    assert got["tests_that_hit_total"] == 757728                        # the parent's, to the test
    assert floor["tests_that_hit_total"] == 757728 and floor["per_brick"]["triangle_tests"] == floor["per_brick"]["tests_that_hit"]
