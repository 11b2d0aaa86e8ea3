"""The product's access routines (csrc/dxv_access.h, compiled for the CPU by tests/access_host.py: the start word, the tile relaxation, the touch
test, the tally, the radius word, driven serially over tiles, tile by tile and in a shuffled tile order; the intrusion map by the thickness's
own stages) against the restatements (tests/access_restated.py), as bytes: A == the widest-path search and the threshold form, I == the
definition, histograms and tally, at every even side 2 .. 26 for both kinds and both connectivities, with and without the culls; on the
builders with the three kinds of seeds; the touch test by itself; the same routines once under AddressSanitizer and UBSan in a program of their
own; and the boundary: header, binding, option, documents.  No GPU."""
import os
import re
import subprocess

import numpy as np
import pytest

import access_host as ah
import access_restated as ar
import flood_seeds as fs
import grid_sides as gs
import thickness_host as th

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIDES = list(range(2, 27, 2))


def smallest_member(g, of):
    m = np.flatnonzero(ar.members(g, of).reshape(-1))
    return m[:1].astype(np.uint32)


@pytest.mark.parametrize("N", SIDES)
def test_host_library_equals_the_restatements_at_every_side(N):
    seen = 0
    for name, g in gs.grids(N):
        seen += 1
        for of in (ar.SOLID, ar.EMPTY):
            for connectivity in (6, 26):
                for seeds in ("border", smallest_member(g, of)):
                    key = (N, name, of, connectivity, type(seeds))
                    got = ah.access(g, of, connectivity, 65, seeds)
                    A = ar.access(g, of, connectivity, 65, seeds)
                    assert got["A"].tobytes() == A.tobytes() == ar.access_by_thresholds(g, of, connectivity, 65, seeds).tobytes(), key
                    assert got["I"].tobytes() == ar.intrusion(g, of, A).tobytes(), key
                    assert got["hist_a"].tobytes() == ar.histogram(A, 65).tobytes() and got["hist_i"].tobytes() == ar.histogram(got["I"], 65).tobytes(), key
                    assert got["tally"] == ar.tally(g, of, A, seeds), key
                    assert got["rounds"] >= 1 and (got["tiles_run"] > 0) == (got["tally"]["seeds_used"] > 0), key
                    other = ah.access(g, of, connectivity, 65, seeds, cull=0, shuffle=N + connectivity)
                    assert other["A"].tobytes() == A.tobytes() and other["I"].tobytes() == got["I"].tobytes() and other["tally"] == got["tally"], key
    assert seen == (5 if N >= 6 else 4)


@pytest.mark.parametrize("connectivity", [6, 26])
@pytest.mark.parametrize("of", [ar.SOLID, ar.EMPTY])
def test_host_library_equals_the_restatement_with_a_seed_in_every_tile(of, connectivity):
    """The seeding of tests/test_gpu_flood_wide_rounds.py, which takes the host library for its expectation at side 162: one member of every
    8^3 tile of "random 0.3" (tests/flood_seeds.py), so round 0 runs every tile.  Side 66 (729 tiles, rows of two words, partial last tiles) is
    the largest of the sweep's residues at which the widest-path search stays within seconds -- measured: solid 0.5 s (6) and 2.5 s (26),
    empty 2.3 s and 5.9 s; at 50 it takes 0.2 .. 2.6 s, and the host library 0.8 .. 1.5 s at 162.  The items take 0.7 .. 5.0 s."""
    N = 66
    g = dict(gs.grids(N, ("random 0.3",)))["random 0.3"]
    seeds = fs.tile_seeds(g, of, 3 + connectivity)
    assert len(np.unique(fs.tile_of(seeds, N))) == len(seeds) == 9 ** 3 and ar.members(g, of).reshape(-1)[seeds].all()
    got = ah.access(g, of, connectivity, 65, seeds)
    A = ar.access(g, of, connectivity, 65, seeds)
    assert got["A"].tobytes() == A.tobytes() and got["I"].tobytes() == ar.intrusion(g, of, A).tobytes(), (of, connectivity)
    assert got["hist_a"].tobytes() == ar.histogram(A, 65).tobytes() and got["hist_i"].tobytes() == ar.histogram(got["I"], 65).tobytes()
    assert got["tally"] == ar.tally(g, of, A, seeds) and got["tally"]["seeds_used"] == 9 ** 3 and got["tiles_run"] >= 9 ** 3
    masked = ah.access(g, of, connectivity, 65, fs.seed_mask(seeds, N), shuffle=connectivity)
    assert masked["A"].tobytes() == A.tobytes() and masked["I"].tobytes() == got["I"].tobytes() and masked["tally"] == got["tally"]


@pytest.mark.parametrize("name", [b[0] for b in ar.builders()])
def test_host_library_on_the_builders_with_the_three_kinds_of_seeds(name):
    _, g, listed = next(b for b in ar.builders() if b[0] == name)
    rng = np.random.default_rng(5)
    mask = (rng.random(g.shape) < 0.02).astype(np.uint8) * 0x40
    for of in (ar.SOLID, ar.EMPTY):
        for connectivity in (6, 26):
            for seeds in ("border", np.array(listed, np.uint32), mask):
                for cap in (2, 65):
                    key = (name, of, connectivity, cap)
                    got = ah.access(g, of, connectivity, cap, seeds, shuffle=3)
                    A = ar.access(g, of, connectivity, cap, seeds)
                    assert got["A"].tobytes() == A.tobytes() and got["I"].tobytes() == ar.intrusion(g, of, A).tobytes() and got["tally"] == ar.tally(g, of, A, seeds), key
                    plain = ah.access(g, of, connectivity, cap, seeds, intrusion=False)
                    assert plain["I"] is None and plain["A"].tobytes() == A.tobytes() and plain["hist_a"].tobytes() == got["hist_a"].tobytes(), key


def test_with_every_member_a_seed_the_host_library_gives_the_thickness():
    g = dict(gs.grids(18))["random 0.3"]
    for of in (ar.SOLID, ar.EMPTY):
        for cap in (9, 4096):
            W, hist = th.thickness(g, of, cap)[:2]
            got = ah.access(g, of, 26, cap, np.ones(g.shape, np.uint8))
            assert got["I"].tobytes() == W.tobytes() and got["hist_i"].tobytes() == hist.tobytes() and got["A"].tobytes() == ar.radius(g, of, cap).astype(np.uint32).tobytes()
            assert got["tally"]["seeds_used"] == got["tally"]["reached"]


def test_a_chamber_raised_twice_takes_more_than_one_round():
    g, seed, chamber = ar.raised_twice()
    got = ah.access(g, ar.EMPTY, 6, 4096, np.array([seed, seed], np.uint32))
    assert got["A"][chamber] == 4 and got["rounds"] > 2 and got["tally"]["seeds_used"] == 1


def test_a_risen_voxel_flags_the_tiles_that_hold_a_neighbour_of_it():
    lib = ah.library()
    for connectivity in (6, 26):
        for z in range(8):
            for y in range(8):
                for x in range(8):
                    want = 0
                    for dz, dy, dx in ar.offsets(connectivity):
                        t = ((z + dz) // 8, (y + dy) // 8, (x + dx) // 8)   # -1, 0 or 1 along every axis
                        if t != (0, 0, 0):
                            want |= 1 << ((t[0] + 1) * 9 + (t[1] + 1) * 3 + (t[2] + 1))
                    assert lib.ac_touch(x, y, z, connectivity) == want, (connectivity, x, y, z)


def test_what_the_routines_accept():
    lib = ah.library()
    assert lib.ac_max_n() == 1024
    assert lib.ac_valid(2, 0, 6, 2) == 1 and lib.ac_valid(1024, 1, 26, 4096) == 1
    for bad in ((0, 0, 6, 65), (3, 0, 6, 65), (1026, 0, 6, 65), (16, 2, 6, 65), (16, 0, 18, 65), (16, 0, 6, 1), (16, 0, 6, 4097)):
        assert lib.ac_valid(*bad) == 0, bad


def test_the_host_routines_are_clean_under_the_sanitizers(tmp_path):
    """a program of its own (its own main, nothing loaded into Python) over the builders' grids, written into a file for it, and random grids"""
    exe, grids = tmp_path / "access_sanitize", tmp_path / "builders.bin"
    built = ar.builders()
    with open(grids, "wb") as fh:
        for _, g, listed in built:
            fh.write(np.array([g.shape[0], len(listed)], np.uint32).tobytes() + np.array(listed, np.uint32).tobytes() + np.ascontiguousarray(g, np.uint8).tobytes())
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", str(exe),
                           os.path.join(ROOT, "tests", "cpp", "access_sanitize_main.cpp")])
    r = subprocess.run([str(exe), str(grids)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout[-1000:], r.stderr[-3000:])
    lines = r.stdout.splitlines()
    assert len([l for l in lines if l.startswith("builder")]) == len(built) * 2 * 2 * 3 and len(lines) == (len(built) + 4 * 2) * 2 * 2 * 3
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr


# ---- the boundary ---------------------------------------------------------------------------------------------------------------------------
ENTRIES = ("dxv_access_async", "dxv_access", "dxv_access_device_ptr", "dxv_access_bytes", "dxv_access_download", "dxv_access_histogram_bytes", "dxv_access_histogram_download",
           "dxv_intrusion_device_ptr", "dxv_intrusion_bytes", "dxv_intrusion_download", "dxv_intrusion_histogram_bytes", "dxv_intrusion_histogram_download", "dxv_access_info",
           "dxv_access_work_info")


def read(*parts):
    with open(os.path.join(ROOT, *parts)) as fh:
        return fh.read()


def test_header_and_binding_agree_on_the_entries_and_on_version_7():
    from dxrvoxelizer_amd import _lib
    h = read("include", "dxv.h")
    declared = set(re.findall(r"DXV_API [^;(]*?\b(dxv_(?:access|intrusion)\w*)\(", h))
    assert declared == set(ENTRIES)
    assert declared == {n for n in _lib.SYMBOLS if n.startswith(("dxv_access", "dxv_intrusion"))}
    assert re.search(r"#define DXV_API_VERSION 7\b", h) and _lib.API_VERSION == 7
    assert ("int dxv_access_async(dxv_ctx* ctx, int of, int connectivity, uint32_t cap_sq, int seeds_kind, const void* seeds, uint32_t seed_count, "
            "int want_intrusion);") in h
    assert ("int dxv_access_info(dxv_ctx* ctx, float* ms, uint32_t* rounds, uint64_t* seeds_used, uint64_t* reached, uint64_t* unreached, uint32_t* widest, "
            "uint32_t* widest_voxel);") in h
    assert "int dxv_access_work_info(dxv_ctx* ctx, uint64_t* tiles_run, uint32_t* most_live_tiles, uint32_t* sparse_rounds);" in h


def test_the_library_exports_the_entries(dxvlib):
    for name in ENTRIES:
        assert getattr(dxvlib, name) is not None
    assert dxvlib.dxv_api_version() == 7


def test_the_rule_and_the_option_are_documented():
    import dxrvoxelizer_amd as dxv
    h = read("include", "dxv.h")
    for phrase in ("A(c) = max over paths s = p0, p1, ..., pk = c of members, p0 in S n M, consecutive voxels adjacent under `connectivity`",
                   "I(p) = max { A(c) : c in M, |p - c|^2 < A(c) }", "{A >= t} is the union of the components of {R >= t} under `connectivity` that hold a seed s with R(s) >= t",
                   "I(p) = 1 + max { r2 in 0 .. cap_sq - 1 : p in DILATE_r2({A >= r2 + 1}) }", "This holds for A and NOT for I", "accessrounds 0..64",
                   "on the frame's stream alone only A is, and only if one batch was enough", "`rounds` may differ from run to run"):
        assert phrase in h, phrase
    policy = read("dxrvoxelizer_amd", "csrc", "dxv_policy.h")
    assert re.search(r'\{"accessrounds", in_range\(0, 64\)', policy) and "int accessrounds = 0;" in policy
    design = read("DESIGN.md")
    section = design[design.index("### 4.18"):]
    for phrase in ("accessrounds", "lower bound", "connected set of members", "geometry alone"):
        assert phrase in section, phrase
    integration = read("INTEGRATION.md")
    for phrase in ("What can get in: access and intrusion", "ink-bottle", "depowdering", "percolation"):
        assert phrase in integration, phrase
    readme = read("README.md")
    assert "dxv_access" in readme and "access.hip" in readme and "dxv_access.h" in readme
    assert "access_times.py" in read("tools", "README.md") and os.path.exists(os.path.join(ROOT, "tools", "access_times.py"))
    hpp = read("include", "dxv_voxelizer.hpp")
    for name in ("Access(", "AccessFromDeviceMask(", "AccessField(", "AccessHistogram(", "IntrusionField(", "IntrusionHistogram(", "AccessInfo("):
        assert name in hpp, name
    for name in ("Access", "AccessField", "AccessHistogram", "IntrusionField", "IntrusionHistogram", "AccessInfo"):
        assert callable(getattr(dxv.Voxelizer, name))
    assert callable(dxv.intrusion_curve)
    assert "access.hip" in read("dxrvoxelizer_amd", "build.py")


def test_the_intrusion_curve():
    import dxrvoxelizer_amd as dxv
    diameter, share = dxv.intrusion_curve(np.array([10, 0, 3, 0, 1], np.uint64))
    assert diameter.dtype == np.float32 and np.array_equal(diameter, dxv.thickness_voxels(np.arange(1, 5))) and share.tolist() == [1.0, 1.0, 0.25, 0.25]
    assert dxv.intrusion_curve(np.array([10, 0, 3, 0, 1], np.uint64), 8)[1].tolist() == [0.5, 0.5, 0.125, 0.125]
    assert dxv.intrusion_curve(np.array([10, 0, 0], np.uint64))[1].tolist() == [0.0, 0.0]
