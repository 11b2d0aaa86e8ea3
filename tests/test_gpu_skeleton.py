"""The skeleton graph on the GPU (include/dxv.h: dxv_skeleton*): the device's labels (uint32 per voxel), nodes and branches equal, as bytes, what
the rule gives for the grid -- by the two restatements (tests/skeleton_restated.py: sets, and a walk) and by the host library
(tests/skeleton_host.py: the product's routines run serially, held to the restatements by tests/test_skeleton_rule.py) -- on the smallest shapes
that still reach each mechanism: the figures at 16^3 and at the grid's border, the word seam at 72 and 130, random grids, a grid of thousands of
tiny nodes and branches, weights from another frame, the pipeline on meshes, the prune, the call's discipline."""
import os
import subprocess

import numpy as np
import pytest

import components_restated as cr
import skeleton_host as sh
import skeleton_restated as sr
import thin_restated as tr
import thin_shapes as ts
from raycast_restated import write_grid

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def dxv(dxvlib):
    import dxrvoxelizer_amd
    return dxrvoxelizer_amd


@pytest.fixture(scope="module")
def writer(dxv, bunny):
    """the one Voxelizer, on the bunny, whose frames the grids of this file are written into"""
    vb, ib, _ = bunny
    v = dxv.Voxelizer(0)
    v.InitFromArrays(vb, ib)
    yield v
    v.close()


@pytest.fixture(scope="module")
def figures():
    return dict(sr.figures(16))


def load(v, g):
    v.Voxelize(g.shape[0])
    write_grid(v, g)


def check(v, g, what="", weights=None, host_weights=None, walk=True):
    """Skeleton of the selected frame, which holds g: labels, nodes, branches and the info's counts against the host library and the
    restatements; returns (labels, nodes, branches)"""
    labels, nodes, branches = v.Skeleton(weights)
    want = sh.skeleton(g, host_weights)
    assert labels.dtype == np.uint32 and labels.shape == g.shape and labels.tobytes() == want[0].tobytes(), (what, int(np.count_nonzero(labels != want[0])))
    assert nodes.dtype == sr.NODE and nodes.tobytes() == want[1].tobytes(), (what, len(nodes), len(want[1]))
    assert branches.dtype == sr.BRANCH and branches.tobytes() == want[2].tobytes(), (what, len(branches), len(want[2]))
    for restated in (sr.by_sets,) + ((sr.by_walk,) if walk else ()):
        r = restated(g, host_weights)
        assert labels.tobytes() == r[0].tobytes() and nodes.tobytes() == r[1].tobytes() and branches.tobytes() == r[2].tobytes(), (what, restated.__name__)
    info = v.SkeletonInfo()
    assert (info["nodes"], info["branches"]) == (len(nodes), len(branches)), (what, info)
    assert (info["end_voxels"], info["curve_voxels"], info["junction_voxels"]) == want[3] == sr.voxel_counts(g), (what, info)
    labels_ptr, nodes_ptr, branches_ptr = v.skeleton_device_ptrs()
    assert labels_ptr and bool(nodes_ptr) == (len(nodes) > 0) and bool(branches_ptr) == (len(branches) > 0), what
    return labels, nodes, branches


# ---- the figures ----------------------------------------------------------------------------------------------------------------------------
def test_a_single_voxel_and_two_voxels(writer, figures):
    v = writer
    load(v, figures["single voxel"])
    _, nodes, branches = check(v, figures["single voxel"], "single voxel")
    assert len(nodes) == 1 and len(branches) == 0 and nodes[0]["voxels"] == 1 and nodes[0]["degree"] == 0 and nodes[0]["flags"] == sr.NODE_END
    write_grid(v, figures["two voxels"])
    _, nodes, branches = check(v, figures["two voxels"], "two voxels")
    assert len(nodes) == 1 and len(branches) == 0 and nodes[0]["voxels"] == 2 and nodes[0]["flags"] == sr.NODE_END


@pytest.mark.parametrize("name, steps", [("segment x", (5, 0, 0)), ("segment y", (5, 0, 0)), ("segment z", (5, 0, 0)), ("plane diagonal", (0, 5, 0)), ("space diagonal", (0, 0, 5))])
def test_segments_have_two_tips_one_branch_and_steps_of_one_type(writer, figures, name, steps):
    v = writer
    load(v, figures[name])
    _, nodes, branches = check(v, figures[name], name)
    assert len(nodes) == 2 and len(branches) == 1 and (nodes["voxels"] == 1).all() and (nodes["degree"] == 1).all()
    assert tuple(branches[0]["steps"]) == steps and branches[0]["voxels"] == 4 and (branches[0]["a"], branches[0]["b"]) == (1, 2)
    assert branches[0]["flags"] == 0                                    # both ends are tips: a free segment, not a spur


def test_closed_branches_the_y_the_theta_the_loop_and_the_square_ring(writer, figures):
    v = writer
    v.Voxelize(16)
    seen = {}
    for name in ("three mutually adjacent", "closed diamond", "Y", "theta", "loop at one node", "square ring"):
        write_grid(v, figures[name])
        seen[name] = check(v, figures[name], name)[1:]
    for name, voxels in (("three mutually adjacent", 3), ("closed diamond", 16)):
        nodes, branches = seen[name]
        assert len(nodes) == 0 and len(branches) == 1 and branches[0]["flags"] == sr.CLOSED and branches[0]["voxels"] == voxels == branches[0]["steps"].sum()
        assert (branches[0]["a"], branches[0]["b"]) == (0, 0)
    nodes, branches = seen["Y"]
    assert len(nodes) == 4 and len(branches) == 3 and sorted(nodes["degree"]) == [1, 1, 1, 3] and ((branches["flags"] & sr.SPUR) != 0).all()
    nodes, branches = seen["theta"]
    assert len(nodes) == 2 and len(branches) == 3 and (nodes["degree"] == 3).all() and (branches["a"] == 1).all() and (branches["b"] == 2).all()
    nodes, branches = seen["loop at one node"]
    loop = branches[branches["a"] == branches["b"]]
    assert len(nodes) == 2 and len(branches) == 2 and len(loop) == 1 and loop[0]["a"] != 0 and nodes[loop[0]["a"] - 1]["degree"] == 3
    nodes, branches = seen["square ring"]
    assert len(nodes) == 4 and (nodes["voxels"] == 2).all() and len(branches) == 8
    assert np.count_nonzero((branches["voxels"] == 1) & (branches["a"] == branches["b"]) & (branches["a"] != 0)) == 4


def test_every_figure_pushed_against_the_border(writer):
    v = writer
    v.Voxelize(16)
    seen = 0
    for name, g in sr.figures(16):
        if "corner" not in name:
            continue
        seen += 1
        write_grid(v, g)
        _, nodes, branches = check(v, g, name)
        assert ((nodes["flags"] & sr.NODE_BORDER) != 0).any() or ((branches["flags"] & sr.BORDER) != 0).any(), name
    assert seen == 26


def test_the_empty_grid_and_the_full_one(writer, figures):
    v = writer
    load(v, figures["empty"])
    _, nodes, branches = check(v, figures["empty"], "empty")
    assert len(nodes) == 0 and len(branches) == 0
    lib, ctx = v._lib, v._ctx
    assert not lib.dxv_skeleton_nodes_device_ptr(ctx) and not lib.dxv_skeleton_branches_device_ptr(ctx)
    assert lib.dxv_skeleton_nodes_bytes(ctx) == 0 and lib.dxv_skeleton_branches_bytes(ctx) == 0 and lib.dxv_skeleton_labels_bytes(ctx) == 4 * 16 ** 3
    write_grid(v, figures["all 0xFF"])
    _, nodes, branches = check(v, figures["all 0xFF"], "all 0xFF")
    assert len(nodes) == 1 and len(branches) == 0 and nodes[0]["voxels"] == 16 ** 3 and nodes[0]["flags"] == sr.NODE_BORDER | sr.NODE_JUNCTION


# ---- word seams -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [72, 130])
def test_figures_across_the_word_seam(writer, N):
    v = writer
    v.Voxelize(N)
    for name, g in sr.seams(N):
        write_grid(v, g)
        labels, nodes, branches = check(v, g, f"{name}, N = {N}")
        assert len(branches) >= 1
    g = dict(sr.seams(N))["branch across the seam"]
    assert tuple(sr.by_sets(g)[2][0]["steps"]) == (11, 0, 0)


# ---- random grids, contention ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [12, 16, 24])
def test_random_grids_with_bytes_other_than_one(writer, N):
    v = writer
    v.Voxelize(N)
    for density in (0.03, 0.1, 0.2):
        g = sr.random_grid(N, density, 7 * N + int(100 * density))
        assert g.max() > 1
        write_grid(v, g)
        _, nodes, branches = check(v, g, f"random {density} at {N}")
        assert len(nodes) > 0 and len(branches) > 0


def test_numbering_under_contention(writer):
    g = sr.contended(32)
    v = writer
    load(v, g)
    _, nodes, branches = check(v, g, "contended")
    assert len(nodes) > 2000 and len(branches) > 500 and np.count_nonzero(branches["flags"] & sr.CLOSED) >= 256


# ---- weights --------------------------------------------------------------------------------------------------------------------------------
def test_weights_from_another_frames_thickness_map(dxv, writer):
    v = writer
    g = sr.random_grid(24, 0.1, 5)
    try:
        v.SetFrame(1)
        load(v, g)
        W = v.Thickness(dxv.COMP_SOLID, 4096)
        ptr = v.thickness_device_ptr()
        v.SetFrame(0)
        load(v, g)
        labels, nodes, branches = check(v, g, "thickness as weights", weights=ptr, host_weights=W)
        for b in range(len(branches)):                                  # a host gather through the labels
            w = W[labels == (sr.BRANCH_BIT | (b + 1))].astype(np.uint64)
            assert (branches[b]["w_min"], branches[b]["w_max"], branches[b]["w_sum"]) == (w.min(), w.max(), w.sum()), b
        for k in range(len(nodes)):
            assert nodes[k]["w_max"] == W[labels == k + 1].max(), k
        graph = dxv.skeleton_graph(nodes, branches)
        assert np.allclose(graph["mean_radius"], np.sqrt(branches["w_sum"] / branches["voxels"])) and (graph["len345"] == sr.len345(branches)).all()
    finally:
        v.SetFrame(0)


def test_weights_whose_sum_needs_64_bits(writer, figures):
    import torch
    v = writer
    g = figures["segment x"]
    load(v, g)
    W = np.where(g != 0, 0xFFFFFFFF, 3).astype(np.uint32)
    t = torch.from_numpy(W.view(np.int32)).cuda()
    _, nodes, branches = check(v, g, "weights of 0xFFFFFFFF", weights=t, host_weights=W)
    assert branches[0]["voxels"] == 4 and branches[0]["w_sum"] == 4 * 0xFFFFFFFF > 2 ** 32 and branches[0]["w_min"] == 0xFFFFFFFF == nodes[0]["w_max"]


def test_weights_that_are_refused(dxv, writer, figures):
    import torch
    v = writer
    g = figures["Y"]
    load(v, g)
    before = check(v, g, "Y")
    good = torch.zeros(16 ** 3 + 1, dtype=torch.int32, device="cuda")
    host = np.zeros(16 ** 3, np.uint32)
    try:
        v.SetFrame(2)                                                   # a map of 8^3 voxels, an allocation of the library's own: too short for 16^3
        load(v, np.ones((8, 8, 8), np.uint8))
        v.Thickness(dxv.COMP_SOLID, 4096)
        short = v.thickness_device_ptr()
    finally:
        v.SetFrame(0)
    for ptr, word in ((good.data_ptr() + 2, "aligned"), (host.ctypes.data, "not device memory"), (short, "the allocation behind")):
        with pytest.raises(dxv.DxvError, match=word):
            v.Skeleton(ptr)
    for got, want in zip((v.SkeletonLabels(), v.SkeletonNodes(), v.SkeletonBranches()), before):       # the earlier skeleton is as it was
        assert got.tobytes() == want.tobytes()


# ---- the pipeline on meshes ------------------------------------------------------------------------------------------------------------------
def test_the_bunny_thinned_to_curves(dxv, writer):
    v = writer
    v.Voxelize(64, dxv.MODE_SURFACE)
    v.Fill()
    v.Thin(dxv.THIN_CURVE)
    labels, nodes, branches = v.Skeleton()
    g = v.Grid()
    want = sr.by_sets(g)
    assert labels.tobytes() == want[0].tobytes() and nodes.tobytes() == want[1].tobytes() and branches.tobytes() == want[2].tobytes()
    host = sh.skeleton(g)
    assert labels.tobytes() == host[0].tobytes() and nodes.tobytes() == host[1].tobytes() and branches.tobytes() == host[2].tobytes()
    assert len(branches) >= 1 and v.SkeletonInfo()["ms"] > 0.0


def test_the_torus_thinned_to_its_kernel_is_one_closed_branch(dxv, writer):
    v = writer
    load(v, ts.torus(32))
    v.Thin(dxv.THIN_KERNEL)
    g = v.Grid()
    _, nodes, branches = check(v, g, "torus kernel")
    assert len(nodes) == 0 and len(branches) == 1 and branches[0]["flags"] & sr.CLOSED
    assert branches[0]["voxels"] == int(np.count_nonzero(g)) == branches[0]["steps"].sum()


# ---- prune ------------------------------------------------------------------------------------------------------------------------------------
def topology(v, dxv):
    v.Components(dxv.COMP_SOLID, 26)
    return v.components_info()[0], int(v.Measure()[0]["euler"])


def test_prune_takes_the_short_arm_at_its_length_and_not_below(dxv, writer, figures):
    v = writer
    g = figures["Y"]
    load(v, g)
    _, nodes, branches = check(v, g, "Y")
    lengths = sorted(sr.len345(branches))
    assert lengths[0] < lengths[1]
    before = topology(v, dxv)
    v.Skeleton()
    v.SkeletonPrune(int(lengths[0]) - 1)
    assert v.SkeletonPruneInfo() == (0, 0) and np.array_equal(v.Grid(), g)
    with pytest.raises(dxv.DxvError, match="stale"):                    # the skeleton went stale with the prune
        v.SkeletonPrune(int(lengths[0]))
    v.Skeleton()
    v.SkeletonPrune(int(lengths[0]))
    got = v.Grid()
    want, gone, voxels = sh.prune(g, int(lengths[0]))
    assert np.array_equal(got, want) and np.array_equal(got, sr.prune(g, int(lengths[0]))[0]) and v.SkeletonPruneInfo() == (gone, voxels) == (1, int(np.count_nonzero(g)) - int(np.count_nonzero(got)))
    assert topology(v, dxv) == before == (len(cr.label(got, cr.SOLID, 26)[1]), tr.euler(got))
    labels, _, _ = check(v, got, "Y pruned")
    short = int(np.argmin(sr.len345(branches)))                         # the spur the first skeleton had at the bound is gone from the second
    assert labels.reshape(-1)[branches[short]["first"]] == 0


def test_a_free_segment_stays_and_two_spurs_at_one_node_go_in_one_pass(dxv, writer, figures):
    v = writer
    g = figures["segment x"]
    load(v, g)
    v.Skeleton()
    v.SkeletonPrune(1000)
    assert np.array_equal(v.Grid(), g) and v.SkeletonPruneInfo() == (0, 0)
    g = figures["Y"]
    write_grid(v, g)
    _, _, branches = check(v, g, "Y")
    lengths = sorted(sr.len345(branches))
    before = topology(v, dxv)
    v.Skeleton()
    v.SkeletonPrune(int(lengths[1]))
    got = v.Grid()
    want, gone, voxels = sh.prune(g, int(lengths[1]))
    assert gone == 2 and np.array_equal(got, want) and np.array_equal(got, sr.prune(g, int(lengths[1]))[0]) and v.SkeletonPruneInfo() == (2, voxels)
    assert topology(v, dxv) == before


def test_pruning_with_a_stale_skeleton_or_none_is_refused(dxv, writer, figures):
    v = writer
    load(v, figures["Y"])
    v.Skeleton()
    v.Voxelize(16)
    write_grid(v, figures["Y"])
    with pytest.raises(dxv.DxvError, match="stale"):
        v.SkeletonPrune(10)
    assert np.array_equal(v.Grid(), figures["Y"])


# ---- discipline -------------------------------------------------------------------------------------------------------------------------------
def test_stale_after_whatever_rewrites_the_grid(dxv, writer, figures):
    v = writer
    g = figures["Y"]
    edits = {"Voxelize": lambda: v.Voxelize(16), "Fill": lambda: v.Fill(), "Morph": lambda: v.Morph(dxv.MORPH_DILATE, 1), "Thin": lambda: v.Thin(dxv.THIN_CURVE),
             "OctreeExpand": lambda: (v.Octree(), v.OctreeExpand()), "SelectComponents": lambda: (v.Components(dxv.COMP_SOLID, 26), v.SelectComponents(dxv.SELECT_LARGEST)),
             "Prune": lambda: v.SkeletonPrune(0)}
    for name, edit in edits.items():
        load(v, g)
        v.Skeleton()
        assert v.skeleton_device_ptrs()[0]
        edit()
        for call in (v.SkeletonLabels, v.SkeletonNodes, v.SkeletonBranches, v.skeleton_device_ptrs):
            with pytest.raises(dxv.DxvError, match="stale"):
                call()
        assert v._lib.dxv_skeleton_labels_bytes(v._ctx) == 0 and v.SkeletonInfo()["nodes"] == 0, name


def test_a_slab_launch_is_refused_and_two_frames_hold_their_own(dxv, writer, figures):
    v = writer
    try:
        v.Voxelize(16, z0=4, nz=8)
        with pytest.raises(dxv.DxvError, match="whole grid"):
            v.Skeleton()
        load(v, figures["Y"])
        first = check(v, figures["Y"], "Y in frame 0")
        v.SetFrame(1)
        load(v, figures["theta"])
        second = check(v, figures["theta"], "theta in frame 1")
        v.SetFrame(0)
        for got, want in zip((v.SkeletonLabels(), v.SkeletonNodes(), v.SkeletonBranches()), first):
            assert got.tobytes() == want.tobytes()
        v.trim()                                                        # the scratch goes, labels and tables stay
        for got, want in zip((v.SkeletonLabels(), v.SkeletonNodes(), v.SkeletonBranches()), first):
            assert got.tobytes() == want.tobytes()
        v.SetFrame(1)
        for got, want in zip((v.SkeletonLabels(), v.SkeletonNodes(), v.SkeletonBranches()), second):
            assert got.tobytes() == want.tobytes()
        v.SetFrame(0)
        v.SkeletonPrune(1000)                                           # a prune reads labels and tables alone: after the trim too
        assert np.array_equal(v.Grid(), sh.prune(figures["Y"], 1000)[0])
    finally:
        v.SetFrame(0)


def test_the_frames_other_products_stay_current_and_unchanged(dxv, writer):
    v = writer
    g = sr.random_grid(16, 0.2, 3)
    load(v, g)
    D = v.DistanceField(dxv.DIST_SQ_I32)
    W = v.Thickness(dxv.COMP_SOLID, 4096)
    L, table = v.Components(dxv.COMP_SOLID, 26)
    check(v, g, "beside other products")
    assert np.array_equal(v.Grid(), g)
    assert v.ThicknessField().tobytes() == W.tobytes() and v.ComponentLabels().tobytes() == L.tobytes() and v.ComponentTable().tobytes() == table.tobytes()
    assert v.Distance().tobytes() == D.tobytes()


# ---- the C++ mirror --------------------------------------------------------------------------------------------------------------------------
def test_cpp_mirror(dxv, bunny, tmp_path):
    vb, ib, _ = bunny
    np.ascontiguousarray(vb, np.float32).tofile(tmp_path / "vb.bin")
    np.ascontiguousarray(ib, np.uint32).tofile(tmp_path / "ib.bin")
    rocm = "/opt/rocm"
    exe = tmp_path / "skeleton_mirror"
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-D__HIP_PLATFORM_AMD__", "-I" + os.path.join(rocm, "include"),
                           os.path.join(ROOT, "tests", "cpp", "skeleton_mirror.cpp"), "-o", str(exe),
                           "-L" + os.path.join(ROOT, "dxrvoxelizer_amd"), "-l:libdxv.so", "-L" + os.path.join(rocm, "lib"), "-lamdhip64",
                           "-Wl,-rpath," + os.path.join(ROOT, "dxrvoxelizer_amd"), "-Wl,-rpath," + os.path.join(rocm, "lib")])
    out = [str(tmp_path / n) for n in ("grid.bin", "labels.bin", "nodes.bin", "branches.bin", "pruned.bin")]
    r = subprocess.run([str(exe), str(tmp_path / "vb.bin"), str(tmp_path / "ib.bin"), "48", "20"] + out, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    g = np.fromfile(out[0], np.uint8).reshape(48, 48, 48)
    labels, nodes, branches, counts = sh.skeleton(g)
    assert np.fromfile(out[1], np.uint32).tobytes() == labels.tobytes() and np.fromfile(out[2], sr.NODE).tobytes() == nodes.tobytes()
    assert np.fromfile(out[3], sr.BRANCH).tobytes() == branches.tobytes()
    pruned, gone, voxels = sh.prune(g, 20)
    assert np.fromfile(out[4], np.uint8).tobytes() == pruned.tobytes()
    lines = [[int(t) for t in line.split()] for line in r.stdout.splitlines()]
    assert len(lines) == 3 and lines[0] == [len(nodes), len(branches)] + list(counts) and lines[1] == [gone, voxels]
    assert sum(lines[2][2:]) <= int(np.count_nonzero(pruned))
