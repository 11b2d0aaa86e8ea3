"""The sparse voxel octree rule (include/dxv.h: dxv_octree) on the CPU: the hand cases of the rule word for word, the numpy
restatement (tests/octree_restated.py) there and back, the product's routines (csrc/dxv_octree.h compiled for the CPU and driven in the
kernels' order: tests/octree_host.py) against the restatement byte for byte, and the checked descent on trees that cannot be followed."""
import os
import re
import subprocess

import numpy as np
import pytest

import grid_sides as gs
import octree_host as oh
import octree_restated as orr
from conftest import ROOT

SIDES = sorted(set(gs.SWEEP) | {2, 4, 6, 8, 30, 66})                   # every even side to 72 (tests/grid_sides.py): partial 8^3 bricks of every size


def as_pairs(nodes):
    return [(int(a), int(b)) for a, b in nodes]


@pytest.mark.parametrize("build", [orr.build, oh.build], ids=["restatement", "host"])
def test_hand_cases_word_for_word(build):
    nodes, first = build(np.zeros((8, 8, 8), np.uint8))
    assert as_pairs(nodes) == [(0, 0x0000)] and first == [0, 1, 1, 1]
    nodes, first = build(np.zeros((2, 2, 2), np.uint8))
    assert as_pairs(nodes) == [(0, 0x0000)] and first == [0, 1]
    nodes, first = build(np.full((8, 8, 8), 0xFF, np.uint8))
    assert as_pairs(nodes) == [(0, 0xFF00)] and first == [0, 1, 1, 1]
    one = np.zeros((8, 8, 8), np.uint8)
    one[7, 0, 3] = 1
    nodes, first = build(one)
    assert as_pairs(nodes) == [(1, 0x0010), (2, 0x0020), (0, 0x2000)] and first == [0, 1, 2, 3]
    nodes, first = build(np.ones((6, 6, 6), np.uint8))                  # S = 8: the octant at the origin is full, seven hold the grid's border
    assert first == [0, 1, 8, 8] and as_pairs(nodes)[0] == (1, 0x01FE)
    for o in range(1, 8):                                               # level-1 cell o: full holds the octants whose level-2 cell lies inside the grid
        inside = sum(1 << c for c in range(8) if all(2 * (o >> a & 1) + (c >> a & 1) < 3 for a in range(3)))
        assert as_pairs(nodes)[o] == (0, inside << 8), o


def grids(N):
    return list(orr.rule_grids(N)) + list(gs.grids(N))


@pytest.mark.parametrize("N", SIDES)
def test_restatement_there_and_back(N):
    for what, g in grids(N):
        nodes, first = orr.build(g)
        L = orr.levels_of(N)
        assert len(first) == L + 1 and first[0] == 0 and first[-1] == len(nodes) and sorted(first) == first, what
        assert (nodes[:, 1] >> 16 == 0).all() and (nodes[first[L - 1]:, 1] & 0xFF == 0).all() and (nodes[first[L - 1]:, 0] == 0).all(), what
        assert np.array_equal(orr.expand(nodes, L, N), (g != 0).astype(np.uint8)), what


@pytest.mark.parametrize("N", SIDES)
def test_host_compiled_build_and_lookup_equal_restatement(N):
    for what, g in grids(N):
        want, wfirst = orr.build(g)
        got, gfirst = oh.build(g)
        assert gfirst == wfirst, what
        assert got.shape == want.shape and np.array_equal(got, want), what
        back, refused = oh.expand(want, orr.levels_of(N), N)
        assert refused == 0 and np.array_equal(back, (g != 0).astype(np.uint8)), what


def test_ball_collapses_over_several_levels_and_shell_does_not():
    N = 66
    ball, _ = orr.build(orr.ball(N))
    assert (ball[:, 1] >> 8 != 0).sum() > 0 and len(ball) * 8 < N ** 3 // 8
    _, first = orr.build(orr.ball(64, 31.9))
    full_by_level = [int((orr.build(orr.ball(64, 31.9))[0][first[l]:first[l + 1], 1] >> 8 != 0).sum()) for l in range(6)]
    assert sum(1 for n in full_by_level if n) >= 3, full_by_level       # full cells of at least three sizes


def test_lookup_refuses_malformed_trees_without_reading_outside_the_array():
    one = np.zeros((8, 8, 8), np.uint8)
    one[7, 0, 3] = 1
    good, _ = orr.build(one)                                            # [(1, 0x10), (2, 0x20), (0, 0x2000)]
    assert oh.lookup_guarded(good, 3, 3, 0, 7) == oh.FULL and oh.lookup_guarded(good, 3, 2, 0, 7) == oh.EMPTY
    assert oh.lookup_guarded(good, 3, 0, 0, 0) == oh.EMPTY

    def tree(pairs):
        return np.array(pairs, np.uint32)

    equal = tree([(1, 0x0010), (3, 0x0020), (0, 0x2000)])               # a child index equal to the node count
    assert oh.lookup_guarded(equal, 3, 3, 0, 7) == oh.BAD
    assert oh.lookup_guarded(equal, 3, 0, 0, 0) == oh.EMPTY             # (what does not pass the index is answered)
    beyond = tree([(0xFFFFFFFF, 0x00FF)])                               # an index beyond it, as far as 32 bits go: index + popcount does not wrap
    for x, y, z in ((0, 0, 0), (7, 7, 7), (4, 0, 0)):
        assert oh.lookup_guarded(beyond, 3, x, y, z) == oh.BAD
    assert oh.lookup_guarded(tree([(0xFFFFFFF9, 0x00FF)]), 3, 7, 7, 7) == oh.BAD      # 0xFFFFFFF9 + 7 = 2^32
    assert oh.lookup_guarded(tree([(1, 0x0010), (7, 0x0020), (0, 0x2000)]), 3, 3, 0, 7) == oh.BAD
    itself = tree([(0, 0x0001)])                                        # a node pointing at itself: the descent ends after L levels
    assert oh.lookup_guarded(itself, 3, 0, 0, 0) == oh.BAD
    assert oh.lookup_guarded(itself, 11, 0, 0, 0) == oh.BAD
    assert oh.lookup_guarded(itself, 3, 1, 0, 0) == oh.EMPTY and oh.lookup_guarded(itself, 3, 4, 0, 0) == oh.EMPTY     # (octant 1 of the last / first step: not flagged)
    loop = tree([(1, 0x0001), (0, 0x0001)])                             # two nodes pointing at each other
    assert oh.lookup_guarded(loop, 4, 0, 0, 0) == oh.BAD
    deep = tree([(1, 0x0010), (2, 0x0020), (0, 0x2020)])                # a level-(L - 1) node that calls a voxel mixed (full wins where both are set)
    assert oh.lookup_guarded(deep, 3, 3, 0, 7) == oh.FULL
    assert oh.lookup_guarded(tree([(1, 0x0010), (2, 0x0020), (0, 0x0020)]), 3, 3, 0, 7) == oh.BAD
    grid, refused = oh.expand(equal, 3, 8)                              # the whole grid: the refused voxels are empty, the rest is answered
    assert refused == 8 and not grid.any()


def test_morton_and_dense_layout_of_the_header():
    L = oh.library()
    rng = np.random.default_rng(3)
    g = np.zeros((66, 66, 66), np.uint8)
    g[tuple(rng.integers(0, 66, (3, 40)))] = 1
    assert np.array_equal(oh.build(g)[0], orr.build(g)[0])              # (oc_build returns 2 where oct_morton and oct_unmorton disagree)
    assert L is not None


# ---- the boundary ----------------------------------------------------------------------------------------------------------------
ENTRIES = {"dxv_octree_async", "dxv_octree", "dxv_octree_info", "dxv_octree_device_ptr", "dxv_octree_bytes", "dxv_octree_download",
           "dxv_octree_ms", "dxv_octree_expand_async", "dxv_octree_expand"}


def test_header_declares_the_octree_entries(tmp_path):
    text = open(os.path.join(ROOT, "include", "dxv.h")).read()
    names = set(re.findall(r"DXV_API\s+[\w\s\*]+?\b(dxv_\w+)\s*\(", text))
    assert ENTRIES <= names
    assert re.search(r"#define DXV_API_VERSION 7\b", text)             # new entries only: no signature or struct changed
    src = tmp_path / "use.c"
    src.write_text('#include "dxv.h"\n'
                   'int main(void) { dxv_ctx* c = 0; float f = 0; uint32_t l = 0, n = 0, first[12];\n'
                   '  return dxv_octree_async(c) + dxv_octree(c) + dxv_octree_info(c, &l, &n, first) + (dxv_octree_device_ptr(c) != 0)\n'
                   '       + (int)dxv_octree_bytes(c) + dxv_octree_download(c, first, sizeof first) + dxv_octree_ms(c, &f)\n'
                   '       + dxv_octree_expand_async(c, 0, 0, 0) + dxv_octree_expand(c, first, 1, 3); }\n')
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), "-c", str(src),
                           "-o", str(tmp_path / "use.o")])
    from dxrvoxelizer_amd import _lib
    assert _lib.API_VERSION == 7 and ENTRIES <= set(_lib.SYMBOLS)
    import dxrvoxelizer_amd
    for method in ("Octree", "OctreeInfo", "OctreeNodes", "octree_device_ptr", "octree_ms", "OctreeExpand"):
        assert callable(getattr(dxrvoxelizer_amd.Voxelizer, method))
    mirror = open(os.path.join(ROOT, "include", "dxv_voxelizer.hpp")).read()
    assert "dxv_octree_async" in mirror and "dxv_octree_expand_async" in mirror and "DownloadOctree" in mirror
