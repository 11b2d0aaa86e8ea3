"""The product's partition routines (csrc/dxv_partition.h, compiled for the CPU by tests/partition_host.py) against the numpy restatement
(tests/partition_restated.py, form (a)), as bytes -- labels, table and throats, both kinds: every side of the sweep at a small cap, noise, blobs,
a torus and a thin sheet, the two grids whose reach crosses 2 and 8 bricks, every value of partprune and the centres in three orders; the same
routines once under AddressSanitizer and UBSan in a program of their own; and the boundary: header, binding, options, documents.  No GPU."""
import os
import re
import subprocess

import numpy as np
import pytest

import grid_sides as gs
import partition_host as ph
import partition_restated as pr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def same(got, want, what):
    for g, w, name in zip(got, want, ("labels", "table", "throats")):
        assert g.dtype == w.dtype and g.shape == w.shape and g.tobytes() == w.tobytes(), (what, name)


@pytest.mark.parametrize("N", gs.SWEEP)
def test_host_library_equals_restatement_at_every_side(N):
    seen = 0
    for name, g in gs.grids(N):
        for of in (pr.SOLID, pr.EMPTY):
            want = pr.partition(g, of, 10)
            for prune in range(4):
                same(ph.partition(g, of, 10, prune), want, (N, name, of, prune))
            seen += 1
    assert seen == (10 if N >= 6 else 8)


GRIDS = {"blobs": lambda: pr.balls(24, 7, count=6, rmax=6), "noise 0.3": lambda: pr.noise(24, 0.3, 1), "noise 0.6": lambda: pr.noise(24, 0.6, 2), "torus": lambda: pr.torus(),
         "sheet": lambda: pr.sheet(18)}


@pytest.mark.parametrize("name", sorted(GRIDS))
def test_shapes_under_every_prune_and_order(name):
    g = GRIDS[name]()
    for of in (pr.SOLID, pr.EMPTY):
        for cap in (1, 17):
            want = pr.partition(g, of, cap)
            for prune in range(4):
                for order in (ph.FORWARD, ph.REVERSED, ph.SHUFFLED):
                    same(ph.partition(g, of, cap, prune, order), want, (name, of, cap, prune, order))
            bare = ph.partition(g, of, cap, want_throats=False)
            assert bare[0].tobytes() == want[0].tobytes() and len(bare[2]) == 0 and not bare[1]["throats"].any()
            stripped = want[1].copy()
            stripped["throats"] = 0
            assert bare[1].tobytes() == stripped.tobytes(), (name, of, cap)


@pytest.mark.parametrize("N,cap", [(40, 101), (72, 1025)])
def test_where_the_reach_crosses_bricks_and_the_coarse_level_matters(N, cap):
    g = pr.balls(40, 3, count=8, rmax=12) if N == 40 else pr.ball_beside_blobs()
    for of in (pr.SOLID, pr.EMPTY):
        want = pr.partition(g, of, cap)
        assert int(want[1]["radius_sq"].max()) > (64 if N == 40 else 256)       # balls that reach across 2, across 4 and more bricks
        tests = []
        for prune in range(4) if N == 40 else (1, 3):                   # (the plain walk of the large grid is the sanitizer program's kind of run, not this one's)
            got = ph.partition(g, of, cap, prune)
            same(got, want, (N, of, cap, prune))
            tests.append(got[3])
        assert all(t[0] == tests[0][0] == int(want[2]["faces"].sum()) for t in tests)
        if N == 40:
            assert tests[3][2] * 4 < tests[0][2] and tests[0][1] == 0, tests     # the pruned search tests a fraction of the plain walk's voxels


def test_the_host_routines_are_clean_under_the_sanitizers(tmp_path):
    exe = tmp_path / "partition_sanitize"
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", str(exe),
                           os.path.join(ROOT, "tests", "cpp", "partition_sanitize_main.cpp")])
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout[-1000:], r.stderr[-3000:])
    assert len(r.stdout.splitlines()) == 4 * 2 * 3 * 2 and "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr


# ---- the boundary ---------------------------------------------------------------------------------------------------------------------------
ENTRIES = ("dxv_partition_async", "dxv_partition", "dxv_partition_info", "dxv_partition_labels_device_ptr", "dxv_partition_labels_bytes", "dxv_partition_labels_download",
           "dxv_partition_table_device_ptr", "dxv_partition_table_bytes", "dxv_partition_table_download", "dxv_partition_throats_device_ptr", "dxv_partition_throats_bytes",
           "dxv_partition_throats_download", "dxv_partition_stage_info")


def read(*parts):
    with open(os.path.join(ROOT, *parts)) as fh:
        return fh.read()


def test_header_and_binding_agree_on_the_entries_and_on_version_7():
    from dxrvoxelizer_amd import _lib
    h = read("include", "dxv.h")
    declared = set(re.findall(r"DXV_API [^;(]*?\b(dxv_partition\w*)\(", h))
    assert declared == set(ENTRIES)
    assert declared == {n for n in _lib.SYMBOLS if n.startswith("dxv_partition")}
    assert re.search(r"#define DXV_API_VERSION 7\b", h) and _lib.API_VERSION == 7
    assert re.search(r"int dxv_partition_async\(dxv_ctx\* ctx, int of, uint32_t cap_sq, int want_throats\);", h)
    assert re.search(r"int dxv_partition\(dxv_ctx\* ctx, int of, uint32_t cap_sq, int want_throats\);", h)
    assert re.search(r"int dxv_partition_info\(dxv_ctx\* ctx, float\* ms, uint32_t\* regions, uint32_t\* throats, uint64_t\* interface_faces\);", h)
    assert re.search(r"int dxv_partition_stage_info\(dxv_ctx\* ctx, float ms\[6\], uint64_t\* cells_tested, uint64_t\* voxels_tested\);", h)
    for name in ("labels", "table", "throats"):
        assert re.search(rf"const void\* dxv_partition_{name}_device_ptr\(const dxv_ctx\* ctx\);", h)
        assert re.search(rf"size_t dxv_partition_{name}_bytes\(const dxv_ctx\* ctx\);", h)
        assert re.search(rf"int dxv_partition_{name}_download\(dxv_ctx\* ctx, void\* host, size_t bytes\);", h)


def test_the_library_exports_the_entries(dxvlib):
    for name in ENTRIES:
        assert getattr(dxvlib, name) is not None
    assert dxvlib.dxv_api_version() == 7


def test_the_rule_and_the_options_are_documented():
    h = read("include", "dxv.h")
    for phrase in ("parent(c) = the highest voxel of the CLOSED ball", "u above v   iff R(u) > R(v), or R(u) == R(v) and index(u) < index(v)",
                   "uint32 root, radius_sq (= R(root)), voxels, throats; uint16 lo[3], hi[3]", "uint32 a, b, faces, neck_sq, neck_voxel", "need not be a 6-connected set",
                   "at least the largest radius^2", "about its diameter long", "partprune 0..3", "partstages 0|1", "1 <= cap_sq <= 4096", "`throats` word, which is 0"):
        assert phrase in h, phrase
    rule = read("dxrvoxelizer_amd", "csrc", "dxv_partition.h")
    for phrase in ("need not be a 6-connected set", "cap_sq bounds the search's reach", "about its diameter long"):
        assert phrase in rule, phrase
    policy = read("dxrvoxelizer_amd", "csrc", "dxv_policy.h")
    assert re.search(r'\{"partprune", in_range\(0, 3\)', policy) and "int partprune = 3;" in policy and re.search(r'\{"partstages", kOnOff', policy)
    design = read("DESIGN.md")
    assert "### 4.16" in design and "partprune" in design and "maximal-ball partition" in design.lower()
    integration = read("INTEGRATION.md")
    assert "Pores, parts and throats" in integration and "Partition(" in integration
    for phrase in ("need not be", "at least the largest radius", "about its diameter long"):
        assert phrase in integration, phrase
    readme = read("README.md")
    assert "dxv_partition" in readme and "partition.hip" in readme and "dxv_partition.h" in readme
    hpp = read("include", "dxv_voxelizer.hpp")
    for name in ("Partition(", "PartitionLabels(", "PartitionTable(", "PartitionThroats(", "PartitionInfo("):
        assert name in hpp, name
    from dxrvoxelizer_amd import build
    assert "partition.hip" in build.SOURCES and "dxv_partition.h" in build.HEADERS


def test_the_python_records_and_the_network_helper():
    import dxrvoxelizer_amd as dxv
    assert dxv.PART_REGION == pr.REGION and dxv.PART_THROAT == pr.THROAT and dxv.PART_REGION.itemsize == 32 and dxv.PART_THROAT.itemsize == 20
    labels, table, throats = pr.partition(pr.dumbbell(), pr.SOLID, 4096)
    net, want = dxv.pore_network(table, throats), pr.pore_network(table, throats)
    assert set(net) == {"radius", "voxels", "coordination", "pairs", "neck_radius", "faces"}
    for k in net:
        assert np.array_equal(net[k], want[k]) and net[k].dtype == want[k].dtype, k
    assert net["radius"][-2:].tolist() == [50 ** 0.5, 37 ** 0.5] and net["pairs"][-1].tolist() == [5, 6] and net["coordination"].tolist() == [1, 1, 1, 1, 2, 4]
    none = dxv.pore_network(table[:0], throats[:0])
    assert none["pairs"].shape == (0, 2) and len(none["radius"]) == 0
    for name in ("Partition", "PartitionLabels", "PartitionTable", "PartitionThroats", "PartitionInfo"):
        assert callable(getattr(dxv.Voxelizer, name)), name
