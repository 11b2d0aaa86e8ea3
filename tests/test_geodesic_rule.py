"""The product's geodesic routines (csrc/dxv_geodesic.h, compiled for the CPU by tests/geodesic_host.py: the tile relaxation, the touch test, the
tally, the descent, driven serially over tiles) against the two restatements (tests/geodesic_restated.py), as bytes: map and tally == (a), the
numpy relaxation, at every side of the sweep up to 40 and == (b), Dijkstra, at every side and the longer rows, for both kinds, both metrics,
border seeds and the single seed [smallest member index], whose front crosses every tile; the path; the limit; the touch test by itself; the same
routines once under AddressSanitizer and UBSan in a program of their own; and the boundary: header, binding, option, documents.  No GPU."""
import os
import re
import subprocess

import numpy as np
import pytest

import flood_seeds as fs
import geodesic_host as gh
import geodesic_restated as gr
import grid_sides as gs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("N", gs.SWEEP + gs.WIDE)
def test_host_library_equals_the_restatements_at_every_side(N):
    seen = 0
    for name, g in gs.grids(N, ("all 0xFF", "ends") if N in gs.WIDE else None):
        seen += 1
        for of in (gr.SOLID, gr.EMPTY):
            for metric in (gr.FACES, gr.CHAMFER):
                for seeds in ("border", gr.smallest_member(g, of)):
                    got, tally, (rounds, tiles) = gh.geodesic(g, of, metric, seeds)
                    want = gr.geodesic_dijkstra(g, of, metric, seeds)
                    assert got.tobytes() == want.tobytes(), (N, name, of, metric, type(seeds))
                    assert tally == gr.tally(want), (N, name, of, metric)
                    if N <= 40:
                        assert got.tobytes() == gr.geodesic(g, of, metric, seeds).tobytes(), (N, name, of, metric)
                    assert rounds >= 1 and (tiles > 0) == (tally["seeds_used"] > 0)
                    if not tally["reached"]:
                        continue
                    far = tally["farthest_voxel"]
                    p = gh.path(got, metric, far)
                    gr.check_path(want, metric, p, far)
                    if metric == gr.FACES:
                        assert len(p) == 1 + tally["farthest"]          # weight 1: a path has as many steps as its length says
                    if N <= 40:
                        assert p.tobytes() == gr.path(want, metric, far).tobytes(), (N, name, of, metric)
    assert seen == (2 if N in gs.WIDE else 5 if N >= 6 else 4)


def test_border_seeds_leave_the_hollow_box_trivial():
    g = dict(gs.grids(24))["hollow box"]                                # its solid lies one voxel inside the border: no seed at all
    out, tally, _ = gh.geodesic(g, gr.SOLID, gr.CHAMFER, "border")
    assert tally["seeds_used"] == 0 and tally["reached"] == 0 and tally["unreached"] == int(np.count_nonzero(g)) and tally["farthest_voxel"] == 0xFFFFFFFF
    out, tally, _ = gh.geodesic(g, gr.EMPTY, gr.FACES, "border")
    assert tally["unreached"] == 20 ** 3                                # the box's inside


@pytest.mark.parametrize("metric", [gr.FACES, gr.CHAMFER])
def test_the_limit_and_a_path_across_many_tiles(metric):
    g = gr.serpentine(24, 1, 1)
    seeds = gr.smallest_member(g, gr.SOLID)
    out0, tally0, (rounds0, tiles0) = gh.geodesic(g, gr.SOLID, metric, seeds)
    assert out0.tobytes() == gr.geodesic_dijkstra(g, gr.SOLID, metric, seeds).tobytes() and tally0["unreached"] == 0
    p = gh.path(out0, metric, tally0["farthest_voxel"])
    assert p.tobytes() == gr.path(out0, metric, tally0["farthest_voxel"]).tobytes() and len(p) > 12 * 20    # twelve slabs, each crossed from one bridge to the next
    gr.check_path(out0, metric, p, tally0["farthest_voxel"])
    occurring = int(np.unique(out0[out0 < gr.UNREACHED])[40])
    for limit in (3, occurring, tally0["farthest"] // 2):
        out, tally, (rounds, tiles) = gh.geodesic(g, gr.SOLID, metric, seeds, limit)
        assert out.tobytes() == gr.limited(out0, limit).tobytes() and tally == gr.tally(out), limit
        assert rounds <= rounds0 and tiles < tiles0                     # the work stays inside the ball
    assert (gr.limited(out0, occurring) == occurring).any()


def test_seed_lists_and_masks():
    g = dict(gs.grids(18))["random 0.3"]
    m = gr.members(g, gr.EMPTY).reshape(-1)
    inside, outside = np.flatnonzero(m), np.flatnonzero(~m)
    idx = np.array([inside[5], inside[900], inside[5], outside[3], inside[-1]], np.uint32)       # a duplicate and a non-member
    mask = np.zeros(18 ** 3, np.uint8)
    mask[idx] = 0x80
    for metric in (gr.FACES, gr.CHAMFER):
        want = gr.geodesic_dijkstra(g, gr.EMPTY, metric, idx)
        for seeds in (idx, mask.reshape(18, 18, 18)):
            out, tally, _ = gh.geodesic(g, gr.EMPTY, metric, seeds)
            assert out.tobytes() == want.tobytes() and tally["seeds_used"] == 3
    out, tally, (rounds, tiles) = gh.geodesic(g, gr.EMPTY, gr.FACES, np.zeros(0, np.uint32))
    assert (rounds, tiles) == (1, 0) and tally["reached"] == 0 and tally["unreached"] == len(inside)


@pytest.mark.parametrize("N, of", [(66, gr.SOLID), (66, gr.EMPTY), (162, gr.SOLID)])
def test_host_library_equals_dijkstra_with_a_seed_in_every_tile(N, of):
    """The seeding of tests/test_gpu_flood_wide_rounds.py, which takes the host library for its expectation at side 162: one member of every
    8^3 tile of "random 0.3" (tests/flood_seeds.py), so round 0 runs every tile -- 9261 at 162, more than the 8192 workgroups of a round's
    launch; 729 at 66.  Measured: at 162 the solid kind takes the host library 1.9 s (FACES) and 2.4 s (CHAMFER) and Dijkstra 0.8 s and 2.5 s;
    the empty kind takes Dijkstra 3.7 s and 8.2 s there (host library 2.7 s and 4.6 s), so it is held at side 66.  The items take 6.7 s (162, solid), 0.6 s
    (66, solid) and 1.4 s (66, empty)."""
    g = dict(gs.grids(N, ("random 0.3",)))["random 0.3"]
    tiles = ((N + 7) // 8) ** 3
    for metric in (gr.FACES, gr.CHAMFER):
        seeds = fs.tile_seeds(g, of, 1 + metric)
        assert len(np.unique(fs.tile_of(seeds, N))) == len(seeds) == tiles and gr.members(g, of).reshape(-1)[seeds].all()
        assert (tiles > fs.ROUND_BLOCKS) == (N == 162)
        assert (fs.tile_seeds(g, of, 7) != seeds).any() and fs.tile_seeds(g, of, 1 + metric).tobytes() == seeds.tobytes()
        got, tally, (rounds, run) = gh.geodesic(g, of, metric, seeds)
        want = gr.geodesic_dijkstra(g, of, metric, seeds)
        assert got.tobytes() == want.tobytes() and tally == gr.tally(want), (N, of, metric)
        assert tally["seeds_used"] == tiles and run >= tiles
        if N == 66:
            assert gh.geodesic(g, of, metric, fs.seed_mask(seeds, N))[0].tobytes() == want.tobytes()


def test_a_changed_voxel_flags_the_tiles_that_hold_a_neighbour_of_it():
    lib = gh.library()
    for metric in (gr.FACES, gr.CHAMFER):
        for z in range(8):
            for y in range(8):
                for x in range(8):
                    want = 0
                    for dz, dy, dx, _ in gr.steps(metric):
                        t = ((z + dz) // 8, (y + dy) // 8, (x + dx) // 8)   # -1, 0 or 1 along every axis
                        if t != (0, 0, 0):
                            want |= 1 << ((t[0] + 1) * 9 + (t[1] + 1) * 3 + (t[2] + 1))
                    assert lib.gc_touch(x, y, z, metric) == want, (metric, x, y, z)


def test_the_largest_grids():
    lib = gh.library()
    assert lib.gc_max_n() == 1024
    assert lib.gc_fits(1024, gr.FACES) == 1 and lib.gc_fits(950, gr.CHAMFER) == 1 and lib.gc_fits(951, gr.CHAMFER) == 0
    assert 5 * (950 ** 3 - 1) < 0xFFFFFFFE <= 5 * (951 ** 3 - 1)


def test_the_host_routines_are_clean_under_the_sanitizers(tmp_path):
    exe = tmp_path / "geodesic_sanitize"
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", str(exe),
                           os.path.join(ROOT, "tests", "cpp", "geodesic_sanitize_main.cpp")])
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout[-1000:], r.stderr[-3000:])
    assert len(r.stdout.splitlines()) == 6 * 2 * 2 * 2 * 3 and "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr


# ---- the boundary ---------------------------------------------------------------------------------------------------------------------------
ENTRIES = ("dxv_geodesic_async", "dxv_geodesic", "dxv_geodesic_device_ptr", "dxv_geodesic_bytes", "dxv_geodesic_download", "dxv_geodesic_info", "dxv_geodesic_work_info",
           "dxv_geodesic_path")


def read(*parts):
    with open(os.path.join(ROOT, *parts)) as fh:
        return fh.read()


def test_header_and_binding_agree_on_the_entries_and_on_version_7():
    from dxrvoxelizer_amd import _lib
    h = read("include", "dxv.h")
    declared = set(re.findall(r"DXV_API [^;(]*?\b(dxv_geodesic\w*)\(", h))
    assert declared == set(ENTRIES)
    assert declared == {n for n in _lib.SYMBOLS if n.startswith("dxv_geodesic")}
    assert re.search(r"#define DXV_API_VERSION 7\b", h) and _lib.API_VERSION == 7
    assert "int dxv_geodesic_async(dxv_ctx* ctx, int of, int metric, int seeds_kind, const void* seeds, uint32_t seed_count, uint32_t limit);" in h
    assert ("int dxv_geodesic_info(dxv_ctx* ctx, float* ms, uint32_t* rounds, uint64_t* seeds_used, uint64_t* reached, uint64_t* unreached, uint32_t* farthest, "
            "uint32_t* farthest_voxel);") in h
    assert "int dxv_geodesic_path(dxv_ctx* ctx, uint32_t target, uint32_t* host_path, uint32_t capacity, uint32_t* length);" in h
    for text in ("DXV_GEO_FACES = 0, DXV_GEO_CHAMFER = 1", "DXV_GEO_SEEDS_BORDER = 0, DXV_GEO_SEEDS_LIST = 1, DXV_GEO_SEEDS_MASK = 2", "#define DXV_GEO_NONE 0xFFFFFFFFu",
                 "#define DXV_GEO_UNREACHED 0xFFFFFFFEu"):
        assert text in h, text


def test_the_library_exports_the_entries(dxvlib):
    for name in ENTRIES:
        assert getattr(dxvlib, name) is not None
    assert dxvlib.dxv_api_version() == 7


def test_the_rule_and_the_option_are_documented():
    import dxrvoxelizer_amd as dxv
    h = read("include", "dxv.h")
    for phrase in ("G(p) = min over paths p0 in S n M, p1, ..., pk = p of allowed steps, of the sum of their weights", "out_limit == where(out_0 <= limit, out_0, UNREACHED) on members",
                   "weight 3 face, 4 edge, 5 corner", "georounds 0..64", "`rounds` may differ from run to run", "wmax (N^3 - 1) < 0xFFFFFFFE", "dz outermost and dx\n * innermost"):
        assert phrase in h, phrase
    policy = read("dxrvoxelizer_amd", "csrc", "dxv_policy.h")
    assert re.search(r'\{"georounds", in_range\(0, 64\)', policy) and "int georounds = 0;" in policy
    design = read("DESIGN.md")
    assert "### 4.15" in design and "georounds" in design and "upper bound" in design[design.index("### 4.15"):]
    assert "Paths, depth and tortuosity" in read("INTEGRATION.md") and "double sweep" in read("INTEGRATION.md")
    assert "dxv_geodesic" in read("README.md") and "geodesic.hip" in read("README.md")
    hpp = read("include", "dxv_voxelizer.hpp")
    for name in ("Geodesic(", "GeodesicField(", "GeodesicInfo(", "GeodesicPath("):
        assert name in hpp, name
    for name in ("Geodesic", "GeodesicInfo", "GeodesicPath", "GeodesicField"):
        assert callable(getattr(dxv.Voxelizer, name))
    assert (dxv.GEO_FACES, dxv.GEO_CHAMFER, dxv.GEO_NONE, dxv.GEO_UNREACHED) == (0, 1, 0xFFFFFFFF, 0xFFFFFFFE)
