"""The exterior flood fill (include/dxv.h: dxv_fill) on the CPU: the numpy restatement (tests/fill_restated.py) on grids whose
answer can be written down, against scipy's labelling where scipy is present, the product's word routines (csrc/dxv_fill.h compiled for the
CPU: tests/fill_host.py) against that restatement, what the header declares, and the kernels' resources."""
import os
import re
import subprocess

import numpy as np
import pytest

import fill_host
import fill_restated as fr
import grid_sides as gs
from conftest import ROOT
from grid_sides import hollow_box

KINDS = (fr.SOLID, fr.INTERIOR)


# ---- the restatement against grids whose answer can be written down --------------------------------------------------------------
def test_restatement_hollow_box_and_a_hole_in_it():
    N = 16
    g = hollow_box(N, 3, 11)
    inside = np.zeros_like(g)
    inside[4:11, 4:11, 4:11] = 1
    assert np.array_equal(fr.fill(g, fr.INTERIOR), inside)
    assert np.array_equal(fr.fill(g, fr.SOLID), g | inside)
    g[3, 7, 6] = 0                                                     # one face voxel removed: the flood gets in
    assert not fr.fill(g, fr.INTERIOR).any()
    assert np.array_equal(fr.fill(g, fr.SOLID), g)


def test_restatement_shell_inside_shell():
    N = 20
    g = hollow_box(N, 2, 17) | hollow_box(N, 6, 12)
    solid = np.zeros_like(g)
    solid[2:18, 2:18, 2:18] = 1                                        # everything within the outer shell, the gap between the two included
    assert np.array_equal(fr.fill(g, fr.SOLID), solid)
    assert np.array_equal(fr.fill(g, fr.INTERIOR), solid & (g == 0))


def test_restatement_edge_contact_does_not_connect():
    N = 8
    g = np.ones((N, N, N), np.uint8)
    g[0, 3, 3] = 0                                                     # free, on the border
    g[1, 4, 3] = 0                                                     # free, touches the first along an edge only
    out = fr.outside(g)
    assert out[0, 3, 3] and not out[1, 4, 3]
    assert fr.fill(g, fr.INTERIOR).sum() == 1 and fr.fill(g, fr.INTERIOR)[1, 4, 3] == 1
    g[1, 5, 4] = 0                                                     # ... and a corner contact from there
    assert not fr.outside(g)[1, 5, 4]
    g[1, 3, 3] = 0                                                     # a face neighbour of both of the first two: now they are joined
    out = fr.outside(g)
    assert out[1, 4, 3] and out[1, 3, 3] and not out[1, 5, 4]


def test_restatement_empty_and_full():
    N = 6
    empty, full = np.zeros((N, N, N), np.uint8), np.full((N, N, N), 0xFF, np.uint8)
    for what in KINDS:
        assert not fr.fill(empty, what).any()
    assert np.all(fr.fill(full, fr.SOLID) == 1) and not fr.fill(full, fr.INTERIOR).any()


def test_restatement_equals_scipy_where_present():
    ndimage = pytest.importorskip("scipy.ndimage")
    for N, density, seed in ((32, 0.3, 1), (48, 0.68, 2), (40, 0.72, 3), (32, 0.95, 4)):
        g = fr.random_walls(N, density, seed)
        labels, _ = ndimage.label(g == 0)                              # default structure: 6-connectivity
        border = np.zeros_like(g, bool)
        border[0] = border[-1] = border[:, 0] = border[:, -1] = border[:, :, 0] = border[:, :, -1] = True
        touching = np.unique(labels[border & (labels != 0)])
        assert np.array_equal(fr.outside(g), np.isin(labels, touching) & (labels != 0)), (N, density)


# ---- the product's routines, compiled for the CPU, against the restatement ---------------------------------------------------------
def check_product(g, name):
    out = fr.outside(g)
    rounds = None
    for what in KINDS:
        want = fr.fill_from(g, out, what)
        for eight in (True, False):                                     # the 8-byte path of pack and write-back, and the byte path
            got, rounds = fill_host.fill(g, what, eight)
            assert got.dtype == np.uint8 and np.array_equal(got, want), (name, what, eight)
    return out, rounds


@pytest.mark.parametrize("density", [0.3, 0.6, 0.68, 0.72, 0.95])
def test_product_routines_equal_restatement_on_random_walls(density):
    g = fr.random_walls(64, density, 64)
    out, _ = check_product(g, f"density {density}")
    assert out.any()
    if density >= 0.6:
        assert (~out & (g == 0)).any()                                 # enclosed pockets exist: the comparison is not an empty one
    check_product(fr.random_walls(30, density, 30, bytes_other_than_one=True), f"bytes, density {density}")


@pytest.mark.parametrize("N", sorted(set(gs.SWEEP) | {2, 4, 30, 64, 66, 96, 130}))     # every even side to 72 (tests/grid_sides.py); rows of one and a half and of three words
def test_product_routines_on_row_lengths(N):
    if N in gs.SWEEP:
        for name, g in gs.grids(N):
            out, _ = check_product(g, f"{N} {name}")
            if name == "hollow box":
                assert int((~out & (g == 0)).sum()) == (N - 4) ** 3
    check_product(fr.random_walls(N, 0.6, N, bytes_other_than_one=True), N)
    g = np.zeros((N, N, N), np.uint8)
    check_product(g, f"{N} empty")
    check_product(g + 0xFF, f"{N} full")
    if N >= 30:
        g = hollow_box(N, 1, N - 2)                                    # a shell one voxel inside the border: its inside spans every word of a row
        out, _ = check_product(g, f"{N} shell")
        assert int((~out & (g == 0)).sum()) == (N - 4) ** 3


def test_product_routines_on_the_baffle_maze():
    g = fr.maze(64)
    out, rounds = check_product(g, "maze")
    assert int(out.sum()) == 119196                                    # nothing is enclosed: every free voxel is outside ...
    assert np.array_equal(fill_host.fill(g, fr.SOLID)[0], g)            # ... and the solid is the walls
    assert rounds > 8                                                  # a path with 31 turns: more rounds than any default batch holds


def test_fill_word_fills_whole_runs():
    L = fill_host.library()
    rng = np.random.default_rng(7)
    for _ in range(2000):
        f = int(rng.integers(0, 1 << 63, dtype=np.uint64)) | (int(rng.integers(0, 2)) << 63)
        r = int(rng.integers(0, 1 << 63, dtype=np.uint64)) & int(rng.integers(0, 1 << 63, dtype=np.uint64)) & f
        want, run = 0, []
        for b in range(65):
            if b < 64 and (f >> b) & 1:
                run.append(b)
            else:
                if any((r >> k) & 1 for k in run):
                    want |= sum(1 << k for k in run)
                run = []
        assert L.fc_fill_word(r, f) == want, (hex(r), hex(f))


# ---- the boundary ----------------------------------------------------------------------------------------------------------------------
def test_header_declares_the_fill_entries(tmp_path):
    text = open(os.path.join(ROOT, "include", "dxv.h")).read()
    names = set(re.findall(r"DXV_API\s+[\w\s\*]+?\b(dxv_\w+)\s*\(", text))
    assert {"dxv_fill_async", "dxv_fill", "dxv_fill_info"} <= names
    assert re.search(r"#define DXV_API_VERSION 7\b", text)             # new entries only: no signature or struct changed
    src = tmp_path / "use.c"
    src.write_text('#include "dxv.h"\n'
                   'int main(void) { dxv_ctx* c = 0; float ms = 0; uint32_t rounds = 0; int a[DXV_FILL_SOLID == 0 && DXV_FILL_INTERIOR == 1 ? 1 : -1]; (void)a;\n'
                   '  return dxv_fill_async(c, DXV_FILL_SOLID) + dxv_fill(c, DXV_FILL_INTERIOR) + dxv_fill_info(c, &ms, &rounds) + dxv_fill_info(c, 0, 0); }\n')
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), "-c", str(src),
                           "-o", str(tmp_path / "use.o")])
    from dxrvoxelizer_amd import _lib
    import dxrvoxelizer_amd as dxv
    assert _lib.API_VERSION == 7 and {"dxv_fill_async", "dxv_fill", "dxv_fill_info"} <= set(_lib.SYMBOLS)
    assert (dxv.FILL_SOLID, dxv.FILL_INTERIOR) == (0, 1)
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), "-x", "c++", "-"], check=True,
                   input=b'#include "dxv_voxelizer.hpp"\nint main() { Voxelizer v; float ms; uint32_t r; return v.Fill() + v.Fill(DXV_FILL_INTERIOR, false) + v.FillInfo(ms, r); }\n')


def test_option_fillrounds_is_a_row_of_the_table_and_a_line_of_the_header():
    L = fill_host.library()
    assert L.fc_option_default(b"fillrounds") == 0
    for v in (0, 1, 4, 64):
        assert L.fc_option_accepts(b"fillrounds", v) == 1, v
    for v in (-1, 65, 1 << 40):
        assert L.fc_option_accepts(b"fillrounds", v) == 0, v
    assert L.fc_option_accepts(b"plan", 2) == 1 and L.fc_option_accepts(b"nosuchoption", 0) == -1      # the other keys are found as before
    assert 1 <= L.fc_default_rounds() <= 64
    header = open(os.path.join(ROOT, "include", "dxv.h")).read()
    doc = header[header.index("Tuning knobs"):header.index("DXV_API int dxv_set_option")]
    assert re.search(r"^ \*\s+fillrounds 0\.\.64\s", doc, re.M)


def test_fill_kernels_use_no_scratch_memory(dxvlib):
    from dxrvoxelizer_amd import build
    if not os.path.exists(os.path.join(build.OBJDIR, "fill.usage")):
        build.build(force=True)
    res = {k: v for k, v in build.kernel_resources("fill").items() if "k_fill" in k}
    assert len(res) == 4, sorted(res)                                  # pack, rows, columns, write
    for k, v in res.items():
        assert v["scratch"] == 0, k
        assert v["lds"] == 0, k
