"""The product's skeleton routines (csrc/dxv_skeleton.h with csrc/dxv_components.h's union-find, compiled for the CPU by tests/skeleton_host.py:
the word's classification from its 26 planes, the first parents over the two masks, the merges, the ranks of the two kinds of roots, the stats
and the tables, driven serially) against the two restatements (tests/skeleton_restated.py), as bytes: on every builder, where the restatements
are held to one another as well, and at every even side 2 .. 26; what deg == 2 promises; the prune's rule and what it keeps; what the routines
accept; the same routines once under AddressSanitizer and UBSan in a program of their own; and the boundary: header, binding, documents.  No GPU."""
import os
import re
import subprocess

import numpy as np
import pytest

import components_restated as cr
import grid_sides as gs
import skeleton_host as sh
import skeleton_restated as sr
import thin_restated as tr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIDES = list(range(2, 27, 2))
BUILDERS = sr.builders()


def same(x, y):
    return all(a.tobytes() == b.tobytes() for a, b in zip(x[:3], y[:3]))


@pytest.mark.parametrize("name", [b[0] for b in BUILDERS])
def test_the_restatements_and_the_host_library_agree_on_every_builder(name):
    g = next(b[1] for b in BUILDERS if b[0] == name)
    sets, walk, host = sr.by_sets(g), sr.by_walk(g), sh.skeleton(g)
    assert sets[0].dtype == np.uint32 and sets[1].dtype == sr.NODE and sets[2].dtype == sr.BRANCH
    assert same(sets, walk) and same(host, sets), name
    assert host[3] == sr.voxel_counts(g) and sum(host[3]) == int(np.count_nonzero(g))
    rng = np.random.default_rng(len(name))
    W = rng.integers(0, 2 ** 32, g.shape, dtype=np.uint64).astype(np.uint32)
    assert same(sr.by_sets(g, W), sr.by_walk(g, W)) and same(sh.skeleton(g, W), sr.by_sets(g, W)), name


@pytest.mark.parametrize("N", SIDES)
def test_host_library_equals_the_restatements_at_every_side(N):
    seen = 0
    for name, g in list(gs.grids(N)) + [("random 0.05", sr.random_grid(N, 0.05, N)), ("random 0.12", sr.random_grid(N, 0.12, N + 1))]:
        seen += 1
        host = sh.skeleton(g)
        assert same(host, sr.by_sets(g)), (N, name)
        if N <= 16 or "0.05" in name:
            assert same(host, sr.by_walk(g)), (N, name)
        assert host[3] == sr.voxel_counts(g), (N, name)
    assert seen == (7 if N >= 6 else 6)


def test_what_degree_two_promises():
    for name, g in BUILDERS:
        labels, nodes, branches = sh.skeleton(g)[:3]
        closed = (branches["flags"] & sr.CLOSED) != 0
        steps = branches["steps"].sum(axis=1)
        assert (steps[closed] == branches["voxels"][closed]).all() and (branches["voxels"][closed] >= 3).all(), name
        assert (steps[~closed] == branches["voxels"][~closed] + 1).all(), name
        assert ((branches["a"] == 0) == closed).all() and (branches["a"] <= branches["b"]).all(), name
        assert int(nodes["degree"].sum()) == 2 * int(np.count_nonzero(~closed)), name
        assert int(nodes["voxels"].sum()) + int(branches["voxels"].sum()) == int(np.count_nonzero(g)), name
        assert (np.diff(nodes["first"].astype(np.int64)) > 0).all() and (np.diff(branches["first"].astype(np.int64)) > 0).all(), name


def test_the_figures_read_as_the_header_says():
    f = dict(sr.figures(16))
    ring = sh.skeleton(f["square ring"])
    assert len(ring[1]) == 4 and (ring[1]["voxels"] == 2).all() and len(ring[2]) == 8
    assert np.count_nonzero((ring[2]["voxels"] == 1) & (ring[2]["a"] == ring[2]["b"]) & (ring[2]["a"] != 0)) == 4
    after = sh.skeleton(tr.thin(f["square ring"], 0)[0])
    assert len(after[1]) == 0 and len(after[2]) == 1 and after[2][0]["flags"] & sr.CLOSED          # Thin(THIN_CURVE) first: one closed branch
    blob = sh.skeleton(np.pad(np.ones((6, 6, 6), np.uint8), 5))
    assert len(blob[1]) == 1 and len(blob[2]) == 0 and blob[1][0]["voxels"] == 216                  # a solid blob is one big node
    loop = sh.skeleton(f["loop at one node"])
    assert ((loop[2]["a"] == loop[2]["b"]) & (loop[2]["a"] != 0)).sum() == 1 and loop[1][0]["degree"] == 3
    segment = sh.skeleton(f["segment x"])
    assert segment[2][0]["flags"] == 0                                  # two tips: a free segment, not a spur


def test_what_the_routines_accept():
    lib = sh.library()
    assert lib.sk_max_n() == 1024
    assert lib.sk_valid(2) == 1 and lib.sk_valid(1024) == 1
    for bad in (0, 1, 3, 1025, 1026, 1624):
        assert lib.sk_valid(bad) == 0, bad


# ---- prune ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["Y", "loop at one node", "segment x", "theta", "random 0.1 at 16", "random 0.03 at 24", "random 0.2 at 12", "contended"])
def test_the_prune_rule(name):
    g = next(b[1] for b in BUILDERS if b[0] == name)
    labels, nodes, branches = sh.skeleton(g)[:3]
    spur = (branches["flags"] & sr.SPUR) != 0
    lengths = sr.len345(branches)
    pieces, euler = len(cr.label(g, cr.SOLID, 26)[1]), tr.euler(g)
    for bound in sorted({0, 8, 15, 0xFFFFFFFF} | {int(v) for v in lengths[spur][:2]} | {int(v) - 1 for v in lengths[spur][:2]}):
        got, gone, voxels = sh.prune(g, bound)
        want, gone2, voxels2 = sr.prune(g, bound)
        assert np.array_equal(got, want) and (gone, voxels) == (gone2, voxels2), (name, bound)
        assert gone == int(np.count_nonzero(spur & (lengths <= bound))) and voxels == int(np.count_nonzero(g)) - int(np.count_nonzero(got)), (name, bound)
        assert (got[got != 0] == g[got != 0]).all()                    # nothing else is touched
        assert len(cr.label(got, cr.SOLID, 26)[1]) == pieces and tr.euler(got) == euler, (name, bound)     # a collapse
        second = sh.skeleton(got)[0].reshape(-1)
        for b in np.flatnonzero(spur & (lengths <= bound)):             # no spur at or below the bound that the first had is in the second
            assert second[branches[b]["first"]] == 0, (name, bound, b)
    if name == "segment x":
        assert np.array_equal(sh.prune(g, 0xFFFFFFFF)[0], g)           # a free segment is never removed


# ---- the sanitizers ---------------------------------------------------------------------------------------------------------------------------
def test_the_host_routines_are_clean_under_the_sanitizers(tmp_path):
    """a program of its own (its own main, nothing loaded into Python) over the builders' grids, written into a file for it, and random grids"""
    exe, grids = tmp_path / "skeleton_sanitize", tmp_path / "builders.bin"
    with open(grids, "wb") as fh:
        for _, g in BUILDERS:
            fh.write(np.array([g.shape[0]], np.uint32).tobytes() + np.ascontiguousarray(g, np.uint8).tobytes())
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wno-unknown-pragmas", "-o", str(exe),
                           os.path.join(ROOT, "tests", "cpp", "skeleton_sanitize_main.cpp")])
    r = subprocess.run([str(exe), str(grids)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout[-1000:], r.stderr[-3000:])
    lines = r.stdout.splitlines()
    assert len([l for l in lines if l.startswith("builder")]) == len(BUILDERS) * 2 and len(lines) == (len(BUILDERS) + 5 * 2) * 2
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr


# ---- the boundary ---------------------------------------------------------------------------------------------------------------------------
ENTRIES = ("dxv_skeleton_async", "dxv_skeleton", "dxv_skeleton_info", "dxv_skeleton_labels_device_ptr", "dxv_skeleton_labels_bytes", "dxv_skeleton_labels_download",
           "dxv_skeleton_nodes_device_ptr", "dxv_skeleton_nodes_bytes", "dxv_skeleton_nodes_download", "dxv_skeleton_branches_device_ptr", "dxv_skeleton_branches_bytes",
           "dxv_skeleton_branches_download", "dxv_skeleton_prune_async", "dxv_skeleton_prune", "dxv_skeleton_prune_info")


def read(*parts):
    with open(os.path.join(ROOT, *parts)) as fh:
        return fh.read()


def test_header_and_binding_agree_on_the_entries_and_on_version_7():
    from dxrvoxelizer_amd import _lib
    h = read("include", "dxv.h")
    declared = set(re.findall(r"DXV_API [^;(]*?\b(dxv_skeleton\w*)\(", h))
    assert declared == set(ENTRIES)
    assert declared == {n for n in _lib.SYMBOLS if n.startswith("dxv_skeleton")}
    assert re.search(r"#define DXV_API_VERSION 7\b", h) and _lib.API_VERSION == 7
    assert "int dxv_skeleton_async(dxv_ctx* ctx, const void* device_weights);" in h
    assert ("int dxv_skeleton_info(dxv_ctx* ctx, float* ms, uint32_t* nodes, uint32_t* branches, uint64_t* end_voxels, uint64_t* curve_voxels, "
            "uint64_t* junction_voxels);") in h
    assert "int dxv_skeleton_prune_async(dxv_ctx* ctx, uint32_t max_len345);" in h
    assert "int dxv_skeleton_prune_info(dxv_ctx* ctx, uint32_t* branches_removed, uint64_t* voxels_removed);" in h


def test_the_library_exports_the_entries(dxvlib):
    for name in ENTRIES:
        assert getattr(dxvlib, name) is not None
    assert dxvlib.dxv_api_version() == 7


def test_the_binding_records_are_the_restatements():
    import dxrvoxelizer_amd as dxv
    assert dxv.SKELETON_NODE == sr.NODE and dxv.SKELETON_BRANCH == sr.BRANCH and dxv.SKELETON_BRANCH_BIT == sr.BRANCH_BIT
    assert (dxv.SKELETON_CLOSED, dxv.SKELETON_BORDER, dxv.SKELETON_SPUR) == (sr.CLOSED, sr.BORDER, sr.SPUR)
    for name in ("Skeleton", "SkeletonLabels", "SkeletonNodes", "SkeletonBranches", "SkeletonInfo", "SkeletonPrune", "SkeletonPruneInfo"):
        assert callable(getattr(dxv.Voxelizer, name))


def test_the_skeleton_graph_of_tables():
    import dxrvoxelizer_amd as dxv
    f = dict(sr.figures(16))
    g = f["Y"]
    W = np.where(g != 0, 9, 0).astype(np.uint32)
    _, nodes, branches = sr.by_sets(g, W)
    graph = dxv.skeleton_graph(nodes, branches, h=0.5)
    s = branches["steps"].astype(np.float64)
    assert np.allclose(graph["length"], 0.5 * (s[:, 0] + np.sqrt(2) * s[:, 1] + np.sqrt(3) * s[:, 2])) and (graph["len345"] == sr.len345(branches)).all()
    assert graph["pairs"].tolist() == [[1, 3], [2, 3], [3, 4]] and graph["spur"].all() and not graph["closed"].any()
    assert np.allclose(graph["mean_radius"], 1.5) and np.allclose(graph["min_radius"], 1.5) and graph["degree"].tolist() == [1, 1, 3, 1] and graph["tip"].tolist() == [True, True, False, True]
    plain = dxv.skeleton_graph(*sr.by_sets(f["closed diamond"])[1:])
    assert plain["closed"].tolist() == [True] and np.isnan(plain["mean_radius"]).all() and plain["pairs"].tolist() == [[0, 0]] and len(plain["degree"]) == 0
    empty = dxv.skeleton_graph(np.zeros(0, dxv.SKELETON_NODE), np.zeros(0, dxv.SKELETON_BRANCH))
    assert empty["pairs"].shape == (0, 2) and len(empty["length"]) == 0


def test_the_rule_and_the_recipes_are_documented():
    h = read("include", "dxv.h")
    for phrase in ("curve(p)   iff deg(p) == 2;   node voxel iff deg(p) != 2   (0: isolated, 1: end, >= 3: junction)",
                   "node       a 26-connected component of the node voxels;   numbered 1 .. K by ascending smallest index",
                   "a path has exactly two attachments (a one-voxel path has both of them)", "uint32 a, b, first, voxels, steps[3], flags; uint32 w_min, w_max; uint64 w_sum",
                   "it is a graph of the shape only for a grid dxv_thin has left", "A solid blob is one big node", "3 steps[0] + 4 steps[1] + 5 steps[2] <= max_len345",
                   "dxv_thin; dxv_skeleton; dxv_skeleton_prune(L); dxv_thin; dxv_skeleton"):
        assert phrase in h, phrase
    design = read("DESIGN.md")
    assert "deg(p) == 2" in design[design.index("## 2"):design.index("## 3")]
    section = design[design.index("### 4.19"):]
    for phrase in ("k_skel_classify", "carry-save", "saturates at 3", "§4.10", "launch_comp_merge"):
        assert phrase in section, phrase
    integration = read("INTEGRATION.md")
    for phrase in ("Skeleton()", "SkeletonPrune", "thickness_device_ptr", "skeleton_graph"):
        assert phrase in integration, phrase
    assert "its ends, its curves and its junctions" not in integration
    readme = read("README.md")
    assert "dxv_skeleton" in readme and "skeleton.hip" in readme and "dxv_skeleton.h" in readme
    hpp = read("include", "dxv_voxelizer.hpp")
    for name in ("Skeleton(", "SkeletonInfo(", "SkeletonPrune("):
        assert name in hpp, name
    assert "skeleton.hip" in read("dxrvoxelizer_amd", "build.py")
