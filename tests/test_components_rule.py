"""Connected components (include/dxv.h: dxv_components*) on the CPU: the numpy restatement (tests/components_restated.py)
against scipy's labelling where scipy is present and on grids whose answer can be written down, the product's routines (csrc/
dxv_components.h compiled for the CPU: tests/components_host.py) run single-threaded as the whole pipeline against that restatement, the
select rules on a table, and what the header declares."""
import os
import re
import subprocess

import numpy as np
import pytest

import components_host as ch
import components_restated as cr
import fill_restated as fr
import grid_sides as gs
from conftest import ROOT

KINDS = (cr.SOLID, cr.EMPTY)
CONNECTIVITIES = (6, 26)
DENSITIES = (0.2, 0.3, 0.6, 0.68)


def row(record):
    return (int(record["first"]), int(record["voxels"]), record["lo"].tolist(), record["hi"].tolist(), int(record["flags"]))


# ---- the restatement ------------------------------------------------------------------------------------------------------------------
def test_restatement_equals_scipy_where_present():
    ndimage = pytest.importorskip("scipy.ndimage")
    grids = [(f"random {N} {d}", fr.random_walls(N, d, N)) for N, d in ((32, 0.3), (24, 0.6), (32, 0.68))] + [("maze 32", fr.maze(32))]
    for what, g in grids:
        for of in KINDS:
            for conn, rank in ((6, 1), (26, 3)):
                want, K = ndimage.label(cr.members(g, of), structure=ndimage.generate_binary_structure(3, rank))
                labels, table = cr.label(g, of, conn)
                assert len(table) == K and np.array_equal(labels, want.astype(np.uint32)), (what, of, conn)
                if K:
                    assert np.array_equal(table["voxels"], np.bincount(want.ravel(), minlength=K + 1)[1:]), (what, of, conn)
                    boxes = ndimage.find_objects(want)
                    assert all(tuple(table["lo"][k][::-1]) == tuple(s.start for s in boxes[k]) and
                               tuple(table["hi"][k][::-1]) == tuple(s.stop - 1 for s in boxes[k]) for k in range(K)), (what, of, conn)


def test_restatement_on_grids_whose_answer_can_be_written_down():
    N = 8
    g = np.zeros((N, N, N), np.uint8)
    g[1, 1, 1] = g[1, 2, 2] = 1                                         # two voxels that share an edge only
    g[5, 5, 5] = g[6, 6, 6] = 0x80                                      # ... and two that share a corner only
    labels, table = cr.label(g, cr.SOLID, 6)
    assert len(table) == 4 and [int(labels[p]) for p in ((1, 1, 1), (1, 2, 2), (5, 5, 5), (6, 6, 6))] == [1, 2, 3, 4]
    labels, table = cr.label(g, cr.SOLID, 26)
    assert len(table) == 2 and [int(labels[p]) for p in ((1, 1, 1), (1, 2, 2), (5, 5, 5), (6, 6, 6))] == [1, 1, 2, 2]
    assert row(table[0]) == (73, 2, [1, 1, 1], [2, 2, 1], 0) and row(table[1]) == (365, 2, [5, 5, 5], [6, 6, 6], 0)
    labels, table = cr.label(g, cr.EMPTY, 6)
    assert len(table) == 1 and row(table[0]) == (0, N ** 3 - 4, [0, 0, 0], [7, 7, 7], 1) and int((labels == 0).sum()) == 4
    assert len(cr.label(np.zeros((N, N, N), np.uint8), cr.SOLID, 6)[1]) == 0
    board = cr.checkerboard(N)
    assert len(cr.label(board, cr.SOLID, 6)[1]) == N ** 3 // 2 and len(cr.label(board, cr.SOLID, 26)[1]) == 1


# ---- the product's routines, compiled for the CPU, against the restatement -----------------------------------------------------------
def check_product(g, what, kinds=KINDS):
    counts = {}
    for of in kinds:
        for conn in CONNECTIVITIES:
            want, wtable = cr.label(g, of, conn)
            for eight, backwards in ((True, False), (False, True)):     # the 8-byte pack and the byte path; the unions in the opposite order
                labels, table = ch.components(g, of, conn, eight, backwards)
                assert labels.dtype == np.uint32 and np.array_equal(labels, want), (what, of, conn, eight)
                assert table.dtype == cr.RECORD and np.array_equal(table, wtable), (what, of, conn, eight)
            counts[of, conn] = len(wtable)
    return counts


@pytest.mark.parametrize("density", DENSITIES)
def test_product_routines_equal_restatement_on_random_walls(density):
    counts = check_product(fr.random_walls(32, density, 32, bytes_other_than_one=True), f"density {density}")
    print(density, counts)
    assert counts[cr.SOLID, 6] > 1 and counts[cr.SOLID, 6] > counts[cr.SOLID, 26] >= 1
    if density >= 0.6:
        assert counts[cr.EMPTY, 6] > 1
    check_product(fr.random_walls(66, density, 66, bytes_other_than_one=True), f"66, density {density}", kinds=(cr.SOLID,) if density < 0.5 else (cr.EMPTY,))


def test_random_grid_has_the_component_counts_that_make_the_comparison_one():
    g = fr.random_walls(32, 0.3, 32)                                    # measured once: 2088 solid components under 6, 14 under 26
    assert len(cr.label(g, cr.SOLID, 6)[1]) > 1000 and 1 < len(cr.label(g, cr.SOLID, 26)[1]) < 100


@pytest.mark.parametrize("N", gs.SWEEP)                                # every even side to 72 (tests/grid_sides.py): rows of less than a word, one word, one word and 2 to 8 bits
def test_product_routines_on_the_sweep_grids(N):
    for name, g in gs.grids(N):
        kinds = KINDS
        if N > 40 and name.startswith("random"):                        # (the restatement takes a second per labelling there: the kind with many components)
            kinds = (cr.EMPTY,) if name == "random 0.6" else (cr.SOLID,)
        counts = check_product(g, f"{N} {name}", kinds=kinds)
        if N >= 8 and name == "random 0.3":
            assert counts[cr.SOLID, 6] > 1


@pytest.mark.parametrize("N", [2, 4, 30, 64, 66])                      # rows of less than a word, one word, one word and two bits
def test_product_routines_on_row_lengths(N):
    z, y, x = np.indices((N, N, N))
    check_product(np.zeros((N, N, N), np.uint8), f"{N} empty")
    check_product(np.full((N, N, N), 0xFF, np.uint8), f"{N} full")
    check_product(cr.one_voxel(N), f"{N} one voxel")
    if N <= 66:
        check_product(cr.checkerboard(N), f"{N} checkerboard", kinds=(cr.SOLID,))
    bars = ((y % 3 == 0) & (z % 2 == 0)).astype(np.uint8)              # runs that span every word of a row, apart from one another
    counts = check_product(bars, f"{N} bars", kinds=(cr.SOLID,))
    assert counts[cr.SOLID, 6] == len(range(0, N, 3)) * len(range(0, N, 2))


def test_rows_of_three_words_against_scipy():
    """N = 130: the restatement's whole-grid steps take minutes there, scipy (which the restatement is checked against above) takes none"""
    ndimage = pytest.importorskip("scipy.ndimage")
    N = 130
    z, y, x = np.indices((N, N, N))
    bars = ((y % 3 == 0) & (z % 2 == 0) & (x != 100)).astype(np.uint8)  # runs over the word boundaries 63 | 64 and 127 | 128
    for what, g in (("bars", bars), ("random", fr.random_walls(N, 0.3, N)), ("full", np.full((N, N, N), 9, np.uint8))):
        for conn, rank in ((6, 1), (26, 3)):
            want, K = ndimage.label(g != 0, structure=ndimage.generate_binary_structure(3, rank))
            labels, table = ch.components(g, cr.SOLID, conn)
            assert len(table) == K and np.array_equal(labels, want.astype(np.uint32)), (what, conn)
            assert np.array_equal(table["voxels"], np.bincount(want.ravel(), minlength=K + 1)[1:]), (what, conn)
            values, where = np.unique(want.ravel(), return_index=True)
            assert np.array_equal(table["first"], where[values > 0]), (what, conn)


def test_a_run_across_the_word_boundary_is_one_component():
    N = 66
    g = np.zeros((N, N, N), np.uint8)
    g[3, 4, 60:66] = 1                                                  # x = 60 .. 65: crosses 63 | 64
    g[7, 7, 63] = g[7, 7, 64] = 2                                       # exactly the two bits at the boundary
    g[9, 9, 63] = g[9, 10, 64] = 3                                      # an edge contact across it: one component under 26 only
    counts = check_product(g, "word boundary", kinds=(cr.SOLID,))
    assert counts[cr.SOLID, 6] == 4 and counts[cr.SOLID, 26] == 3
    labels, table = ch.components(g, cr.SOLID, 6)
    assert row(table[0]) == ((3 * N + 4) * N + 60, 6, [60, 4, 3], [65, 4, 3], 1)


def test_a_u_shape_whose_arms_meet_in_the_last_row_re_roots_a_numbered_run():
    N = 16
    g = np.zeros((N, N, N), np.uint8)
    g[2, 3:12, 9] = 1                                                   # the right arm starts first in linear order ...
    g[2, 5:12, 4] = 1                                                   # ... the left arm later, so the arms have different roots until
    g[2, 11, 4:10] = 1                                                  # the last row joins them: the left arm's root goes under the right's
    counts = check_product(g, "U")
    assert counts[cr.SOLID, 6] == 1 and counts[cr.SOLID, 26] == 1
    labels, table = ch.components(g, cr.SOLID, 6)
    assert row(table[0]) == ((2 * N + 3) * N + 9, 9 + 7 + 4, [4, 3, 2], [9, 11, 2], 0)
    g[2, 11, 6] = 0                                                     # the bridge cut: two components, numbered by their first voxels
    labels, table = ch.components(g, cr.SOLID, 6)
    assert len(table) == 2 and labels[2, 3, 9] == 1 and labels[2, 5, 4] == 2 and labels[2, 11, 5] == 2 and labels[2, 11, 7] == 1


def test_voxels_that_share_only_an_edge_or_only_a_corner():
    """one component under 26, two under 6 -- through the product's routines, every diagonal direction, at the grid's faces and across 63 | 64"""
    N = 8
    g = np.zeros((N, N, N), np.uint8)
    g[1, 1, 1] = g[1, 2, 2] = 1                                         # an edge only
    g[5, 5, 5] = g[6, 6, 6] = 0x80                                      # a corner only
    counts = check_product(g, "edge and corner", kinds=(cr.SOLID,))
    assert counts[cr.SOLID, 6] == 4 and counts[cr.SOLID, 26] == 2
    labels, table = ch.components(g, cr.SOLID, 26)
    assert [int(labels[p]) for p in ((1, 1, 1), (1, 2, 2), (5, 5, 5), (6, 6, 6))] == [1, 1, 2, 2]
    assert row(table[0]) == (73, 2, [1, 1, 1], [2, 2, 1], 0) and row(table[1]) == (365, 2, [5, 5, 5], [6, 6, 6], 0)
    for N, at in ((8, 3), (8, 1), (8, 6), (66, 63), (66, 64)):          # the second voxel at x - 1, x and x + 1; x = 0 and N - 1 reached
        for dz, dy, dx in ((1, 1, -1), (1, -1, 1), (1, -1, -1), (1, 1, 1), (1, 0, -1), (1, 0, 1), (1, -1, 0), (1, 1, 0), (0, 1, -1), (0, 1, 1)):
            g = np.zeros((N, N, N), np.uint8)
            g[2, 3, at] = g[2 + dz, 3 + dy, at + dx] = 7
            counts = check_product(g, f"{N}: {at} and {(dz, dy, dx)}", kinds=(cr.SOLID,))
            assert counts[cr.SOLID, 6] == 2 and counts[cr.SOLID, 26] == 1


def test_product_routines_on_the_baffle_maze():
    counts = check_product(fr.maze(32), "maze")
    assert counts[cr.EMPTY, 6] == 1 and counts[cr.SOLID, 6] == 1


def test_run_start():
    L = ch.library()
    rng = np.random.default_rng(11)
    for _ in range(500):
        m = int(rng.integers(0, 1 << 63, dtype=np.uint64)) | (int(rng.integers(0, 2)) << 63)
        for b in range(64):
            if m >> b & 1:
                s = b
                while s and m >> (s - 1) & 1:
                    s -= 1
                assert L.cc_run_start(m, b) == s, (hex(m), b)
    assert L.cc_run_start((1 << 64) - 1, 63) == 0


# ---- the select rules on a table ------------------------------------------------------------------------------------------------------
def test_select_rules_on_a_table_ties_included():
    t = np.zeros(6, cr.RECORD)
    t["voxels"] = [5, 40, 7, 40, 1, 39]
    t["flags"] = [1, 0, 0, 1, 0, 1]
    for table in (t, t[:1], t[:0]):
        for rule, arg in ((cr.LARGEST, 0), (cr.MIN_VOXELS, 0), (cr.MIN_VOXELS, 7), (cr.MIN_VOXELS, 40), (cr.MIN_VOXELS, 41), (cr.BORDER, 0)):
            assert np.array_equal(ch.select(table, rule, arg), cr.keep(table, rule, arg)), (len(table), rule, arg)
    assert ch.select(t, cr.LARGEST).tolist() == [False, True, False, False, False, False]      # 40 twice: the smaller number
    assert ch.select(t, cr.MIN_VOXELS, 7).tolist() == [False, True, True, True, False, True]
    assert ch.select(t, cr.BORDER).tolist() == [True, False, False, True, False, True]
    g = fr.random_walls(24, 0.3, 5, bytes_other_than_one=True)
    for of in KINDS:
        labels, table = cr.label(g, of, 6)
        for rule, arg in ((cr.LARGEST, 0), (cr.MIN_VOXELS, 3), (cr.BORDER, 0)):
            out, (kept, dropped, changed) = cr.select(g, labels, table, of, rule, arg)
            assert kept + dropped == len(table) and changed == int(((out != 0) != (g != 0)).sum())
            assert np.array_equal(out[labels == 0], g[labels == 0])    # every other byte stays as it is
    labels, table = cr.label(g, cr.EMPTY, 6)
    out, _ = cr.select(g, labels, table, cr.EMPTY, cr.BORDER)
    assert np.array_equal(out != 0, fr.fill(g) != 0)                    # Components(EMPTY, 6); Select(BORDER) is dxv_fill(DXV_FILL_SOLID)'s set


# ---- the boundary ----------------------------------------------------------------------------------------------------------------------
def test_header_declares_the_components_entries(tmp_path):
    text = open(os.path.join(ROOT, "include", "dxv.h")).read()
    names = set(re.findall(r"DXV_API\s+[\w\s\*]+?\b(dxv_\w+)\s*\(", text))
    want = {"dxv_components_async", "dxv_components", "dxv_components_info", "dxv_components_labels_device_ptr", "dxv_components_labels_bytes",
            "dxv_components_table_device_ptr", "dxv_components_table_bytes", "dxv_components_labels_download", "dxv_components_table_download",
            "dxv_components_ms", "dxv_components_select_async", "dxv_components_select", "dxv_components_select_info"}
    assert want <= names
    assert re.search(r"#define DXV_API_VERSION 7\b", text)             # new entries only: no signature or struct changed
    assert ch.library().cc_max_n() == 1624 and 1625 ** 3 < 2 ** 32 < 1626 ** 3
    src = tmp_path / "use.c"
    src.write_text('#include "dxv.h"\n'
                   'int main(void) { dxv_ctx* c = 0; uint32_t k = 0, d = 0; uint64_t v = 0; int of = 0, n = 0; float ms = 0;\n'
                   '  int a[DXV_COMP_SOLID == 0 && DXV_COMP_EMPTY == 1 && DXV_SELECT_LARGEST == 0 && DXV_SELECT_MIN_VOXELS == 1 && DXV_SELECT_BORDER == 2 ? 1 : -1]; (void)a;\n'
                   '  return dxv_components_async(c, DXV_COMP_SOLID, 6) + dxv_components(c, DXV_COMP_EMPTY, 26) + dxv_components_info(c, &k, &of, &n) + dxv_components_ms(c, &ms)\n'
                   '    + (dxv_components_labels_device_ptr(c) != 0) + (dxv_components_table_device_ptr(c) != 0) + (int)dxv_components_labels_bytes(c) + (int)dxv_components_table_bytes(c)\n'
                   '    + dxv_components_labels_download(c, 0, 0) + dxv_components_table_download(c, 0, 0) + dxv_components_select_async(c, DXV_SELECT_LARGEST, 0)\n'
                   '    + dxv_components_select(c, DXV_SELECT_MIN_VOXELS, 40) + dxv_components_select_info(c, &k, &d, &v); }\n')
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), "-c", str(src), "-o", str(tmp_path / "use.o")])
    from dxrvoxelizer_amd import _lib
    import dxrvoxelizer_amd as dxv
    assert _lib.API_VERSION == 7 and want <= set(_lib.SYMBOLS)
    assert (dxv.COMP_SOLID, dxv.COMP_EMPTY, dxv.SELECT_LARGEST, dxv.SELECT_MIN_VOXELS, dxv.SELECT_BORDER) == (0, 1, 0, 1, 2)
    assert dxv.COMP_RECORD == cr.RECORD and dxv.COMP_RECORD.itemsize == 24
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), "-x", "c++", "-"], check=True,
                   input=b'#include "dxv_voxelizer.hpp"\nint main() { Voxelizer v; uint32_t k, d; uint64_t c; int of, n; float ms; std::vector<uint32_t> l; '
                         b'std::vector<Voxelizer::ComponentRecord> t;\n return v.Components(0) + v.Components(1, DXV_COMP_EMPTY, 26) + v.ComponentsInfo(k, of, n) + '
                         b'v.DownloadComponents(l, t) + v.ComponentsMs(ms) + v.SelectComponents(DXV_SELECT_LARGEST) + v.SelectComponents(DXV_SELECT_MIN_VOXELS, 40, false) + '
                         b'v.SelectInfo(k, d, c) + (v.DeviceComponentLabels() != nullptr) + (v.DeviceComponentTable() != nullptr); }\n')
