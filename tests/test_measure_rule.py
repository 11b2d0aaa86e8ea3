"""The product's measure routines (csrc/dxv_measure.h, compiled for the CPU by tests/measure_host.py: every mask word, every run, plain additions)
against the numpy restatement (tests/measure_restated.py), as bytes: at every side of the sweep and the three longer rows, for both kinds and
both connectivities; under the flips and permutations of a grid, where the ownership of cells at connectivity 26 -- which is not symmetric --
would show; single runs against sums written out; and the boundary (header, binding, C++ wrapper).  No GPU."""
import itertools
import os
import re
import subprocess

import numpy as np
import pytest

import components_restated as cr
import fill_restated as fr
import grid_sides as gs
import measure_host as mh
import measure_restated as ms
import thin_shapes as ts

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = list(itertools.product((cr.SOLID, cr.EMPTY), (6, 26)))


def check_product(g, what):
    for of, conn in CASES:
        labelling = ms.label(g, of, conn)
        want = ms.measure(g, of, conn, labelling)
        got = mh.measure(g, of, conn, *labelling)
        assert got.tobytes() == want.tobytes(), (what, of, conn, [n for n in ms.RECORD.names if not np.array_equal(got[n], want[n])])


@pytest.mark.parametrize("N", gs.SWEEP + gs.WIDE)
def test_product_routines_equal_restatement_at_every_side(N):
    """every even side to 72 and the three longer rows.  The random grids stop at side 72: components_restated.label, which the restatement
    falls back to without scipy, takes 0.5 s there, 4.5 s at 126 and 28 s at 194 per labelling of one, and "ends" 20 s at 194; with scipy's
    labelling the longer rows take 1.3 s at 126 and 130 and 6 s at 194, most of it the restatement's cell counts."""
    names = ("all 0xFF", "ends") if N in gs.WIDE else None
    seen = 0
    for name, g in gs.grids(N, names):
        seen += 1
        check_product(g, (N, name))
    assert seen == (2 if N in gs.WIDE else 5 if N >= 6 else 4)


@pytest.mark.parametrize("N", [12, 32])
def test_product_routines_equal_restatement_on_the_shapes(N):
    for name, g in ts.shapes(N):
        check_product(g, (N, name))
    check_product(cr.checkerboard(N), (N, "checkerboard"))
    check_product(cr.one_voxel(N), (N, "one voxel"))
    check_product(np.zeros((N, N, N), np.uint8), (N, "empty"))


def test_flips_and_permutations_of_a_random_grid():
    g = fr.random_walls(20, 0.3, 5, bytes_other_than_one=True)
    for fx, fy, fz in itertools.product((False, True), repeat=3):
        check_product(np.ascontiguousarray(g[::-1 if fz else 1, ::-1 if fy else 1, ::-1 if fx else 1]), ("flip", fx, fy, fz))
    for axes in itertools.permutations(range(3)):
        check_product(np.ascontiguousarray(g.transpose(axes)), ("transpose", axes))


def test_rods_across_the_word_boundaries_of_a_row():
    check_product(ts.rods(130), "rods")


def test_one_run_has_its_moments_in_closed_form_and_its_own_cells():
    for s, length, word in ((0, 64, 0), (63, 1, 1), (5, 17, 2), (0, 1, 0), (1, 62, 25)):
        x0, y, z = 64 * word + s, 1601, 1623
        cur = ((1 << length) - 1) << s
        xs = list(range(x0, x0 + length))
        for conn in (6, 26):
            r = mh.run(0, cur, 0, conn, s, length, x0, y, z)
            assert r["voxels"] == length and r["sum"].tolist() == [sum(xs), length * y, length * z]
            assert r["sum2"].tolist() == [sum(x * x for x in xs), length * y * y, length * z * z]
            assert r["prod"].tolist() == [sum(xs) * y, length * y * z, sum(xs) * z]
            assert r["faces"] == 4 * length + 2 and r["euler"] == 1     # a rod by itself: contractible
            # the same run with members beside it in the words before and behind: no x face at a word's end that a neighbour covers
            r = mh.run(1 << 63, cur, 1, conn, s, length, x0, y, z)
            assert r["faces"] == 4 * length + 2 - (s == 0) - (s + length == 64)
    assert mh.library().mc_max_n() == 1624 and 1623 ** 5 < 2 ** 63      # the largest sum, of ix^2 over a full grid, fits


def test_header_declares_the_measure_entries(tmp_path):
    text = open(os.path.join(ROOT, "include", "dxv.h")).read()
    names = set(re.findall(r"DXV_API\s+[\w\s\*]+?\b(dxv_\w+)\s*\(", text))
    entries = {"dxv_measure_async", "dxv_measure", "dxv_measure_table_device_ptr", "dxv_measure_table_bytes", "dxv_measure_table_download", "dxv_measure_ms"}
    assert entries <= names
    for phrase in ("record 0 is the sum of the others", "No sum overflows for N <= 1624", "#corners - #edges + #faces - #cubes", "v - e + f - c"):
        assert phrase.lower() in text.lower(), phrase
    src = tmp_path / "use.c"
    src.write_text('#include "dxv.h"\n'
                   'int main(void) { dxv_ctx* c = 0; float ms = 0; char t[96];\n'
                   '  return dxv_measure_async(c) + dxv_measure(c) + (dxv_measure_table_device_ptr(c) != 0) + (int)dxv_measure_table_bytes(c)\n'
                   '         + dxv_measure_table_download(c, t, sizeof t) + dxv_measure_ms(c, &ms); }\n')
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), "-c", str(src), "-o", str(tmp_path / "use.o")])
    from dxrvoxelizer_amd import _lib
    import dxrvoxelizer_amd as dxv
    version = int(re.search(r"#define DXV_API_VERSION (\d+)\b", text).group(1))
    assert version == 7 and _lib.API_VERSION == version and entries <= set(_lib.SYMBOLS)
    assert dxv.MEASURE_RECORD == ms.RECORD and dxv.MEASURE_RECORD.itemsize == 96
    for name in ("Measure", "MeasureTable", "measure_device_ptr", "measure_ms", "Betti"):
        assert callable(getattr(dxv.Voxelizer, name)), name
    assert callable(dxv.mass_properties)
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), "-x", "c++", "-"], check=True,
                   input=b'#include "dxv_voxelizer.hpp"\nint main() { Voxelizer v; std::vector<Voxelizer::MeasureRecord> t; uint32_t a, b, c; float ms;\n'
                         b'bool ok = v.Measure() && v.Measure(false) && v.MeasureTable(t) && v.Betti(a, b, c) && v.MeasureMs(ms);\n'
                         b'Voxelizer::MeasureRecord r = {}; return (int)Voxelizer::MassProperties(r).volume + ok; }\n')
