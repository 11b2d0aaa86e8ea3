"""Morphology by the Euclidean ball (include/dxv.h: dxv_morph) on the CPU: the two numpy restatements (tests/morph_restated.py)
against each other, the properties the rule's border convention gives, the sealing example with its numbers, the product's word routines
(csrc/dxv_morph.h compiled for the CPU: tests/morph_host.py) against the restatement, and what the header declares."""
import os
import re
import subprocess

import numpy as np
import pytest

import fill_restated as fr
import grid_sides as gs
import morph_host
import morph_restated as mr
from conftest import ROOT

RADII = (1, 2, 3, 4, 9, 10, 27)
SIDES = (2, 6, 16, 24)


def grids(N):
    z, y, x = np.indices((N, N, N))
    for density in (0.05, 0.5, 0.9):
        yield f"random {density}", fr.random_walls(N, density, 100 + N, bytes_other_than_one=True)
    yield "all zero", np.zeros((N, N, N), np.uint8)
    yield "all 0xFF", np.full((N, N, N), 0xFF, np.uint8)
    yield "checkerboard", ((x + y + z) & 1).astype(np.uint8)
    one = np.zeros((N, N, N), np.uint8)
    one[N - 1, 0, N // 2] = 7
    yield "one voxel", one


# ---- the restatements ------------------------------------------------------------------------------------------------------------------
def test_ball_offset_counts():
    assert [len(mr.ball_offsets(r2)) for r2 in (1, 2, 3, 4)] == [7, 19, 27, 33]
    assert len(mr.ball_offsets(9)) == 123 and (0, 0, 3) in mr.ball_offsets(9) and (1, 1, 3) not in mr.ball_offsets(9)


@pytest.mark.parametrize("N", SIDES)
def test_the_two_restatements_agree(N):
    for what, g in grids(N):
        for r2 in RADII:
            for op in mr.OPS:
                a, b = mr.morph(g, op, r2), mr.morph_by_distance(g, op, r2)
                assert a.dtype == np.uint8 and a.max(initial=0) <= 1 and np.array_equal(a, b), (N, what, r2, op)


@pytest.mark.parametrize("N", SIDES)
def test_close_is_extensive_open_anti_extensive_both_idempotent(N):
    for what, g in grids(N):
        solid = g != 0
        for r2 in RADII:
            closed, opened = mr.morph(g, mr.CLOSE, r2), mr.morph(g, mr.OPEN, r2)
            assert not (solid & (closed == 0)).any(), (N, what, r2)
            assert not (~solid & (opened != 0)).any(), (N, what, r2)
            assert np.array_equal(mr.morph(closed, mr.CLOSE, r2), closed), (N, what, r2)
            assert np.array_equal(mr.morph(opened, mr.OPEN, r2), opened), (N, what, r2)


@pytest.mark.parametrize("N", SIDES)
def test_erode_of_the_all_solid_grid_is_all_solid(N):
    full = np.full((N, N, N), 0xFF, np.uint8)
    for r2 in RADII + (mr.MAX_RADIUS_SQ,):
        assert np.all(mr.morph_by_distance(full, mr.ERODE, r2) == 1), r2
    for r2 in RADII:
        assert np.all(mr.morph(full, mr.ERODE, r2) == 1), r2
        assert not mr.morph(np.zeros_like(full), mr.DILATE, r2).any()


def test_the_sealing_example():
    holed, whole = mr.holed_shell()
    assert int(whole.sum()) - int(holed.sum()) == 32 and int(holed.sum()) == 2952
    leaky = fr.fill(holed)
    assert np.array_equal(leaky, holed) and int(leaky.sum()) == 2952   # the flood gets in: nothing is enclosed
    want = fr.fill(whole)
    assert int(want.sum()) == 7208
    sealed = mr.morph(fr.fill(mr.morph(holed, mr.DILATE, 8)), mr.ERODE, 8)
    assert np.array_equal(sealed, want)
    assert int(mr.morph(fr.fill(mr.morph(holed, mr.DILATE, 4)), mr.ERODE, 4).sum()) == 7188


# ---- the product's routines, compiled for the CPU, against the restatement ------------------------------------------------------------------
def check_product(g, r2, what_for, restate=mr.morph):
    for op in mr.OPS:
        want = restate(g, op, r2)
        for eight in (True, False):                                     # the 8-byte path of pack and write-back, and the byte path
            got, was_set, cleared = morph_host.morph(g, op, r2, eight)
            assert got.dtype == np.uint8 and np.array_equal(got, want), (what_for, r2, op, eight)
            assert (was_set, cleared) == mr.counts(g, want), (what_for, r2, op, eight)


@pytest.mark.parametrize("N", gs.SWEEP)                                # every even side to 72 (tests/grid_sides.py): rows of one word, and of a word and 2 to 8 bits
def test_product_routines_equal_restatement(N):
    if N in (2, 6, 16, 24, 30, 64, 66):
        for what, g in grids(N):
            for r2 in RADII if N <= 30 else (1, 4, 10):
                check_product(g, r2, (N, what))
    for what, g in gs.grids(N):
        for r2 in (1, 10):
            check_product(g, r2, (N, what))


def test_product_routines_at_the_far_end_of_the_range():
    N = 70                                                             # two words per row, the second of six bits
    for axis in range(3):
        for gap, radii in ((64, (4095, 4096)), (65, (4096,))):
            g = np.zeros((N, N, N), np.uint8)
            a, b = [3, 2, 1], [3, 2, 1]                                 # along x the pair lies across the word boundary
            b[2 - axis] = a[2 - axis] + gap
            g[tuple(a)] = 1
            g[tuple(b)] = 0x80
            for r2 in radii:
                for op in (mr.DILATE, mr.ERODE):
                    got, was_set, cleared = morph_host.morph(g, op, r2)
                    want = mr.morph_by_distance(g, op, r2)
                    assert np.array_equal(got, want) and (was_set, cleared) == mr.counts(g, want), (axis, gap, r2, op)
    one = np.zeros((N, N, N), np.uint8)
    one[1, 2, 3] = 1
    for r2, reached in ((4095, 0), (4096, 1)):
        out = morph_host.morph(one, mr.DILATE, r2)[0]
        assert out[65, 2, 3] == reached and out[1, 66, 3] == reached and out[1, 2, 67] == reached, r2
        assert out[64, 2, 3] == 1 and out[1, 2, 66] == 1 and out[1, 2, 68] == 0 and out[66, 2, 3] == 0, r2


def test_word_routines():
    L = morph_host.library()
    assert all(L.mc_isqrt(v) == int(np.floor(np.sqrt(v))) for v in range(0, 4097))
    rng = np.random.default_rng(11)
    for _ in range(300):
        prev, m, nxt = (int(v) for v in rng.integers(0, 1 << 63, 3, dtype=np.uint64) * 2 + rng.integers(0, 2, 3, dtype=np.uint64))
        row = prev | (m << 64) | (nxt << 128)
        for k in (1, 2, 31, 63, 64):
            want = ((row << k) | (row >> k)) >> 64 & ((1 << 64) - 1)
            assert L.mc_shifted(prev, m, nxt, k) == want, (hex(prev), hex(m), hex(nxt), k)


def test_field_form_routines():
    """the threshold of the field form is the identity of the rule, its halves are the operations', and the radius picks the form"""
    import distance_restated as dr
    L = morph_host.library()
    g = fr.random_walls(12, 0.4, 5, bytes_other_than_one=True)
    for grid in (g, np.zeros_like(g), np.full_like(g, 3)):
        d = dr.distance_sq(grid)
        for r2 in (1, 3, 9, 27, 4096):
            for erode, op in ((0, mr.DILATE), (1, mr.ERODE)):
                got = np.array([L.mc_threshold(int(v), r2, erode) for v in d.reshape(-1)], np.uint8).reshape(d.shape)
                assert np.array_equal(got, mr.morph_by_distance(grid, op, r2)), (r2, op)
    assert [[L.mc_half_erodes(op, h) for h in (0, 1)] for op in mr.OPS] == [[0, 0], [1, 1], [1, 0], [0, 1]]
    switch = L.mc_planes_max_radius_sq()
    assert 1024 <= switch < 4096                                        # (profiles/NOTES.md, "Morphology": the planes are no dearer than the field form at 1024, 3 x dearer at 4096)
    assert L.mc_form(switch, 0) == 1 and L.mc_form(switch + 1, 0) == 2 and L.mc_form(1, 0) == 1 and L.mc_form(4096, 0) == 2
    assert L.mc_form(4096, 1) == 1 and L.mc_form(1, 2) == 2


# ---- the boundary ------------------------------------------------------------------------------------------------------------------------
def test_header_declares_the_morph_entries(tmp_path):
    text = open(os.path.join(ROOT, "include", "dxv.h")).read()
    names = set(re.findall(r"DXV_API\s+[\w\s\*]+?\b(dxv_\w+)\s*\(", text))
    entries = {"dxv_morph_async", "dxv_morph", "dxv_morph_info"}
    assert entries <= names
    assert re.search(r"#define DXV_API_VERSION 7\b", text)             # new entries only: no signature or struct changed
    src = tmp_path / "use.c"
    src.write_text('#include "dxv.h"\n'
                   'int main(void) { dxv_ctx* c = 0; float ms = 0; uint64_t s = 0, k = 0;\n'
                   '  int a[DXV_MORPH_DILATE == 0 && DXV_MORPH_ERODE == 1 && DXV_MORPH_OPEN == 2 && DXV_MORPH_CLOSE == 3 ? 1 : -1]; (void)a;\n'
                   '  return dxv_morph_async(c, DXV_MORPH_DILATE, 9u) + dxv_morph(c, DXV_MORPH_CLOSE, 1u) + dxv_morph_info(c, &ms, &s, &k) + dxv_morph_info(c, 0, 0, 0); }\n')
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), "-c", str(src),
                           "-o", str(tmp_path / "use.o")])
    from dxrvoxelizer_amd import _lib
    import dxrvoxelizer_amd as dxv
    assert _lib.API_VERSION == 7 and entries <= set(_lib.SYMBOLS)
    assert (dxv.MORPH_DILATE, dxv.MORPH_ERODE, dxv.MORPH_OPEN, dxv.MORPH_CLOSE) == mr.OPS
    assert callable(dxv.Voxelizer.Morph) and callable(dxv.Voxelizer.morph_info)
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), "-x", "c++", "-"], check=True,
                   input=b'#include "dxv_voxelizer.hpp"\nint main() { Voxelizer v; float ms; uint64_t s, c; return v.Morph(DXV_MORPH_OPEN, 9) + v.Morph(DXV_MORPH_ERODE, 1, false) + v.MorphInfo(ms, s, c); }\n')
