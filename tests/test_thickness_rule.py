"""The product's thickness routines (csrc/dxv_thickness.h, compiled for the CPU by tests/thickness_host.py) against the numpy restatement
(tests/thickness_restated.py, form (a)), as bytes: every side of the sweep with all the sweep's grids and both kinds at cap_sq 6 -- random grids
stay below the cap there and the hollow box's inside reaches it --, all four values of thickcull, a ladder of caps on a 40^3 union of balls; the
same routines once under AddressSanitizer and UBSan in a program of their own; and the boundary: header, binding, option, documents.  No GPU."""
import os
import re
import subprocess

import numpy as np
import pytest

import grid_sides as gs
import thickness_host as th
import thickness_restated as tr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
from thickness_restated import CAP_LADDER, ladder_grid  # noqa: E402


@pytest.mark.parametrize("N", gs.SWEEP)
def test_host_library_equals_restatement_at_every_side(N):
    seen = 0
    for name, g in gs.grids(N):
        for of in (tr.SOLID, tr.EMPTY):
            want = tr.thickness(g, of, 6)
            hist = tr.histogram(want, 6)
            for cull in range(4):
                W, h, (centres, items) = th.thickness(g, of, 6, cull)
                assert W.tobytes() == want.tobytes(), (N, name, of, cull)
                assert h.tobytes() == hist.tobytes(), (N, name, of, cull)
                assert items >= centres, (N, name, of, cull)
            seen += 1
    assert seen == (10 if N >= 6 else 8)


def test_random_grids_stay_below_the_cap_and_the_hollow_box_reaches_it():
    for name, g in gs.grids(24):
        top = int(tr.thickness(g, tr.SOLID, 6).max()), int(tr.thickness(g, tr.EMPTY, 6).max())
        if name.startswith("random"):
            assert max(top) < 6, name
        if name == "hollow box":
            assert top == (1, 6)


@pytest.fixture(scope="module")
def ladder():
    return ladder_grid()


@pytest.mark.parametrize("cap", CAP_LADDER)
def test_cap_ladder_on_a_union_of_balls(ladder, cap):
    for of in (tr.SOLID, tr.EMPTY):
        want = tr.thickness(ladder, of, cap)
        painted = []
        for cull in range(4):
            W, h, counters = th.thickness(ladder, of, cap, cull)
            assert W.tobytes() == want.tobytes(), (cap, of, cull)
            assert h.tobytes() == tr.histogram(want, cap).tobytes(), (cap, of, cull)
            painted.append(counters)
        assert painted[3][0] <= min(painted[1][0], painted[2][0]) and max(painted[1][0], painted[2][0]) <= painted[0][0], (cap, of, painted)
        if cap == 2:
            assert painted[0] == (0, 0)                                 # R is 1 or the cap: nothing is painted voxel by voxel


def test_the_culls_remove_most_centres_of_a_blob():
    g = tr.balls(40, 3, count=8, rmax=12)
    none, both = th.thickness(g, tr.SOLID, 17, 0)[2], th.thickness(g, tr.SOLID, 17, 3)[2]
    assert both[0] * 3 < none[0] and both[1] * 3 < none[1], (none, both)


def test_the_integer_square_root_is_exact():
    lib = th.library()
    for v in list(range(0, 20000)) + [k * k + d for k in range(140, 4097, 97) for d in (-1, 0, 1)]:
        r = lib.tc_isqrt(v)
        assert r * r <= v < (r + 1) * (r + 1), v


def test_the_host_routines_are_clean_under_the_sanitizers(tmp_path):
    exe = tmp_path / "thickness_sanitize"
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", str(exe),
                           os.path.join(ROOT, "tests", "cpp", "thickness_sanitize_main.cpp")])
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout[-1000:], r.stderr[-3000:])
    assert len(r.stdout.splitlines()) == (3 * 4 - 1) * 2 * 2 and "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr


# ---- the boundary ---------------------------------------------------------------------------------------------------------------------------
ENTRIES = ("dxv_thickness_async", "dxv_thickness", "dxv_thickness_device_ptr", "dxv_thickness_bytes", "dxv_thickness_download", "dxv_thickness_histogram_bytes",
           "dxv_thickness_histogram_download", "dxv_thickness_info", "dxv_thickness_stage_info")


def read(*parts):
    with open(os.path.join(ROOT, *parts)) as fh:
        return fh.read()


def test_header_and_binding_agree_on_the_entries_and_on_version_7():
    from dxrvoxelizer_amd import _lib
    h = read("include", "dxv.h")
    declared = set(re.findall(r"DXV_API [^;(]*?\b(dxv_thickness\w*)\(", h))
    assert declared == set(ENTRIES)
    assert declared == {n for n in _lib.SYMBOLS if n.startswith("dxv_thickness")}
    assert re.search(r"#define DXV_API_VERSION 7\b", h) and _lib.API_VERSION == 7
    assert re.search(r"int dxv_thickness_async\(dxv_ctx\* ctx, int of, uint32_t cap_sq\);", h)
    assert re.search(r"int dxv_thickness_info\(dxv_ctx\* ctx, float\* ms, uint64_t\* centres_painted, uint64_t\* work_items\);", h)


def test_the_library_exports_the_entries(dxvlib):
    for name in ENTRIES:
        assert getattr(dxvlib, name) is not None
    assert dxvlib.dxv_api_version() == 7


def test_the_rule_and_the_option_are_documented():
    h = read("include", "dxv.h")
    for phrase in ("W(p)  = max { R(c) : c in M, |p - c|^2 < R(c) }", "1 + max { r2 in 0 .. cap_sq - 1 : p in OPEN(r2) }", "not nested", "thickcull 0..3", "thickstages 0|1", "2 <= cap_sq <= 4096"):
        assert phrase in h, phrase
    policy = read("dxrvoxelizer_amd", "csrc", "dxv_policy.h")
    assert re.search(r'\{"thickcull", in_range\(0, 3\)', policy) and "int thickcull = 3;" in policy
    design = read("DESIGN.md")
    assert "4.14" in design and "thickcull" in design
    assert "Wall thickness and pore size" in read("INTEGRATION.md")
    hpp = read("include", "dxv_voxelizer.hpp")
    for name in ("Thickness(", "ThicknessField(", "ThicknessHistogram(", "ThicknessInfo(", "ThicknessVoxels("):
        assert name in hpp, name


def test_the_python_helper_turns_squared_radii_into_voxels():
    import dxrvoxelizer_amd as dxv
    W = np.array([0, 1, 4, 9, 16, 4096], np.uint32)
    out = dxv.thickness_voxels(W)
    assert out.dtype == np.float32 and out.tolist() == [0.0, 1.0, 3.0, 5.0, 7.0, 127.0]
    assert np.array_equal(out, tr.thickness_voxels(W))
