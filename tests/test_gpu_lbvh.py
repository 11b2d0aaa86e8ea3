"""The LBVH build on the GPU (csrc/lbvh.hip, radix_sort.hip, the header routines behind them) at adversarial triangle counts and keys:
every stage's download against the numpy restatement (tests/lbvh_restated.py) and the product's headers compiled for the host
(tests/hostcheck), word for word; refits over the build's links; walks over these trees against the brute-force oracle.  The inputs and
the branch each reaches: tests/lbvh_meshes.py, DESIGN.md section 4.1.  array_equal throughout: no tolerance anywhere."""
import ctypes as C

import numpy as np
import pytest

import lbvh_meshes as lm
import lbvh_restated as lr
import mesh_distance_restated as mr

pytestmark = pytest.mark.gpu

DBG_SORTED_KEYS, DBG_NODES, DBG_TRI_POS, DBG_TRI_NRM, DBG_PARENTS, DBG_NODES32, DBG_NODES64 = range(7)
RESTATED_UP_TO = 4097                        # the restatement's tree: up to here, and for the highest comb
REFITS = (1, 2, 0)                           # min/max pyramid (default), level sweeps, one atomic climb


@pytest.fixture(scope="module")
def dxv(dxvlib):
    import dxrvoxelizer_amd
    return dxrvoxelizer_amd


class Want:
    """the references of one mesh: the host's run of the product's headers, and the restatement (its tree where the case has one)"""

    def __init__(self, hostcheck, vb, ib, tree):
        self.vb, self.ib = vb, ib
        self.rest = lr.Build(vb, ib, tree=tree)
        self.host = hostcheck(vb, ib, self.rest.bound)
        L = hostcheck.lib
        self.T = self.rest.T
        self.keys, self.nodes, self.nodes32, self.nodes64 = self.host.keys(), self.host.nodes(), self.host.nodes32(), self.host.nodes64()
        self.tripos = np.empty((self.T, 12), np.float32)
        L.hc_scene_tripos.argtypes = [C.c_void_p, C.c_void_p]
        L.hc_scene_tripos(self.host.h, self.tripos.ctypes.data_as(C.c_void_p))
        self.height = self.host.height
        self.parents = lr.parent_words(self.nodes[:, 12:14].view(np.int32)) if self.T > 1 else None


_WANT = {}


def want_of(hostcheck, name, vb=None, ib=None):
    if name not in _WANT:
        if vb is None:
            vb, ib = lm.get(name)
        T = len(ib) // 3
        _WANT[name] = Want(hostcheck, vb, ib, tree=T <= RESTATED_UP_TO or name == "comb-16")
    return _WANT[name]


def traversal_copies(hostcheck, nodes):
    """the host's compress_node / widen_node of exact nodes"""
    L = hostcheck.lib
    L.hc_traversal_copies.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p]
    nodes = np.ascontiguousarray(nodes, np.uint32)
    out32, out64 = np.empty((len(nodes), 8), np.uint32), np.empty((len(nodes), 16), np.uint32)
    L.hc_traversal_copies(nodes.ctypes.data_as(C.c_void_p), len(nodes), out32.ctypes.data_as(C.c_void_p), out64.ctypes.data_as(C.c_void_p))
    return out32, out64


def differ(got, want):
    bad = np.argwhere(np.asarray(got != want).reshape(len(got), -1).any(1)).ravel()
    return f"{len(bad)} rows differ, first {bad[:6].tolist()}"


def check_half_copies(nodes, nodes32, nodes64, tag):
    """the properties of the half-float copies, on the device's own download"""
    assert len(lr.outward_violations(nodes, nodes32)) == 0, (tag, "a half plane is inside the exact box or not the tightest outside it",
                                                             lr.outward_violations(nodes, nodes32)[:6].tolist())
    assert np.array_equal(nodes32[:, 6:8], nodes[:, 12:14]), (tag, "compressed nodes: links")
    assert np.array_equal(lr.wide_from_32(nodes32), nodes64), (tag, "wide nodes are not their children's planes in order", differ(lr.wide_from_32(nodes32), nodes64))


def check_stages(v, w, tag):
    """every download of a fresh build of w's mesh on context v against w"""
    r, T = w.rest, w.T
    st = v.stats()
    assert st["num_tris"] == T and st["num_nodes"] == max(T - 1, 1)
    assert np.array_equal(np.asarray(st["bound"], np.float32).view(np.uint32), r.bound.view(np.uint32)), (tag, "bound")
    keys = v.debug(DBG_SORTED_KEYS)
    assert np.array_equal(keys, r.keys), (tag, "sorted keys differ from the restatement", differ(keys, r.keys))
    assert np.array_equal(keys, w.keys), (tag, "sorted keys differ from the host code")
    tp = v.debug(DBG_TRI_POS)
    index = tp[:, 3].view(np.uint32)
    assert np.array_equal(index, (keys & np.uint64(0xffffffff)).astype(np.uint32)), (tag, "index words are not the keys' low halves")
    assert np.array_equal(np.sort(index), np.arange(T, dtype=np.uint32)), (tag, "index words are not a permutation")
    assert np.array_equal(tp.reshape(T, 3, 4)[:, :, :3].view(np.uint32), r.tri_pos().view(np.uint32)), (tag, "positions differ from the restatement")
    assert np.array_equal(tp[:, 7].view(np.uint32), w.tripos[:, 7].view(np.uint32)), (tag, "class words differ from the host code")
    assert np.array_equal(tp.view(np.uint32), w.tripos.view(np.uint32)), (tag, "triangle records differ from the host code")
    tn = v.debug(DBG_TRI_NRM).reshape(T, 3, 4)
    assert np.array_equal(tn[:, :, :3].view(np.uint32), w.vb[w.ib.reshape(-1, 3)[r.order], 3:6].view(np.uint32)) and not tn[:, :, 3].view(np.uint32).any(), (tag, "normal records")
    nodes = v.debug(DBG_NODES)
    for what, cols in (("links", slice(12, 14)), ("boxes", slice(0, 12)), ("heights", slice(14, 16))):
        assert np.array_equal(nodes[:, cols], w.nodes[:, cols]), (tag, what, "differ from the host code", differ(nodes[:, cols], w.nodes[:, cols]))
        if r.has_tree:
            assert np.array_equal(nodes[:, cols], r.nodes[:, cols]), (tag, what, "differ from the restatement", differ(nodes[:, cols], r.nodes[:, cols]))
    if T > 1:
        parents = v.debug(DBG_PARENTS)
        assert np.array_equal(parents, w.parents), (tag, "parent words", differ(parents, w.parents))
        if r.has_tree:
            assert np.array_equal(parents, r.parents), (tag, "parent words differ from the restatement")
        root = nodes[0, :12].view(np.float32)
        assert np.array_equal(np.minimum(root[0:3], root[6:9]), r.root_lo) and np.array_equal(np.maximum(root[3:6], root[9:12]), r.root_hi), (tag, "root box")
    assert st["tree_height"] == w.height, (tag, "tree height", st["tree_height"], w.height)
    if r.has_tree or T == 1:
        assert st["tree_height"] == r.height, (tag, "tree height against the restatement")
    assert np.float32(st["tri_extent"]).view(np.uint32) == r.tri_extent.view(np.uint32), (tag, "tri_extent", st["tri_extent"], float(r.tri_extent))
    nodes32, nodes64 = v.debug(DBG_NODES32), v.debug(DBG_NODES64)
    assert np.array_equal(nodes32, w.nodes32), (tag, "compressed nodes", differ(nodes32, w.nodes32))
    assert np.array_equal(nodes64, w.nodes64), (tag, "wide nodes", differ(nodes64, w.nodes64))
    check_half_copies(nodes, nodes32, nodes64, tag)


def build_and_check(dxv, w, tag, refits=REFITS):
    v = dxv.Voxelizer(0)
    try:
        v.set_option("wide", 1)
        for refit in refits:
            v.set_option("refit", refit)
            v.InitDynamic(w.vb, w.ib)
            check_stages(v, w, (tag, "refit", refit))
    finally:
        v.close()


# ---- stages ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", lm.NAMES)
def test_build_stages(dxv, hostcheck, name):
    build_and_check(dxv, want_of(hostcheck, name), name)


@pytest.mark.parametrize("name", ["count-1", "count-2", "count-1025", "count-2049", "count-65537", "comb-8"])
def test_build_stages_with_four_sort_passes(dxv, hostcheck, name):
    """digits of 8 bits: four passes over the 30 code bits, an even number, so the keys start in the other buffer"""
    v = dxv.Voxelizer(0)
    try:
        v.set_option("sortbits", 8)                          # (the plan is the process's)
        build_and_check(dxv, want_of(hostcheck, name), (name, "sortbits 8"))
    finally:
        v.set_option("sortbits", 0)
        v.close()


@pytest.mark.parametrize("T", lm.FUSED_BOUNDARY)
def test_build_stages_at_the_fused_launch_boundary(dxv, hostcheck, T):
    """2 097 152: the last count of the fused gather + hierarchy launch and of the sort's small shape (three passes); 2 097 153: two
    launches, the medium shape, four passes.  Host check only."""
    _, vb, ib = lm.fused_boundary(T)
    w = Want(hostcheck, vb, ib, tree=False)
    build_and_check(dxv, w, f"fused-{T}", refits=(1, 2))


# ---- refit ----------------------------------------------------------------------------------------------------------------------
# does a build from the moved vertices have the first build's Morton order and links?  (restated on the CPU, asserted below: only then
# are its boxes comparable with the refit's)
REFIT_CASES = {"count-2": True, "count-3": True, "count-1024": False, "count-1025": False, "count-2049": False, "copies-1025": True,
               "runs": False, "comb-8": False, "comb-12": False, "flat-x": False, "flat-y": False, "flat-z": False}


@pytest.mark.parametrize("name", list(REFIT_CASES))
def test_refit_over_the_builds_links(dxv, hostcheck, name):
    vb, ib = lm.get(name)
    if name.startswith(("count-", "flat-")):
        vb, ib = lm.pinned(vb, ib, 1.5)                      # (the soups reach beyond 1)
    w = want_of(hostcheck, "refit/" + name, vb, ib)
    r = w.rest
    new = lm.moved(vb, ib, seed=7)
    assert np.array_equal(lr.bound_of(new), r.bound)
    want_nodes, root_lo, root_hi = r.refit(new)
    assert not np.array_equal(want_nodes[:, :12], r.nodes[:, :12])
    want32, want64 = traversal_copies(hostcheck, want_nodes)
    want_tp = lr.normalised(new, r.bound)[ib.reshape(-1, 3)[r.order]]
    again = lr.Build(new, ib)
    same = np.array_equal(again.order, r.order) and np.array_equal(again.links, r.links)
    assert same == REFIT_CASES[name]
    v, v2 = dxv.Voxelizer(0), dxv.Voxelizer(0)
    try:
        for x in (v, v2):
            x.set_option("wide", 1)
        for refit, defer in ((1, 0), (1, 1), (2, 1), (0, 1)):
            tag = (name, "refit", refit, "deferboxes", defer)
            v.set_option("refit", refit)
            v.set_option("deferboxes", defer)
            v.InitDynamic(vb, ib)
            nodes0, parents0 = v.debug(DBG_NODES), v.debug(DBG_PARENTS)
            assert np.array_equal(nodes0, r.nodes), (tag, "build", differ(nodes0, r.nodes))
            v.UpdateVertices(new)
            st = v.stats()
            assert st["tree_height"] == r.height and np.array_equal(np.asarray(st["bound"], np.float32), r.bound), tag
            nodes = v.debug(DBG_NODES)
            assert np.array_equal(nodes[:, 12:], nodes0[:, 12:]), (tag, "a refit changed links or heights")
            assert np.array_equal(v.debug(DBG_PARENTS), parents0), (tag, "a refit changed parent words")
            assert np.array_equal(v.debug(DBG_SORTED_KEYS), r.keys), (tag, "a refit changed the keys")
            assert np.array_equal(nodes[:, :12], want_nodes[:, :12]), (tag, "refitted boxes", differ(nodes[:, :12], want_nodes[:, :12]))
            tp = v.debug(DBG_TRI_POS).reshape(-1, 3, 4)
            assert np.array_equal(tp[:, :, :3].view(np.uint32), want_tp.view(np.uint32)), (tag, "refitted triangle records")
            assert np.array_equal(tp[:, 0, 3].view(np.uint32), r.order.astype(np.uint32)), tag
            nodes32, nodes64 = v.debug(DBG_NODES32), v.debug(DBG_NODES64)
            assert np.array_equal(nodes32, want32), (tag, "compressed nodes", differ(nodes32, want32))
            assert np.array_equal(nodes64, want64), (tag, "wide nodes", differ(nodes64, want64))
            check_half_copies(nodes, nodes32, nodes64, tag)
            v2.set_option("refit", refit)
            v2.InitDynamic(new, ib)                           # a build from the moved vertices
            fresh = v2.debug(DBG_NODES)
            assert np.array_equal(fresh, again.nodes), (tag, "second build", differ(fresh, again.nodes))
            if same:
                assert np.array_equal(fresh, nodes), (tag, "a build over the same links gives other boxes than the refit")
    finally:
        v.close()
        v2.close()


# ---- walks over these trees -----------------------------------------------------------------------------------------------------
WALK_CASES = ("count-1", "count-2", "count-3", "count-5", "count-257", "count-1025", "copies-1025", "runs", "comb-7", "comb-8",
              "comb-8-soup", "flat-x", "flat-y", "flat-z", "clamped")
_GRIDS = {}


def oracle_grid(orc, name, mode):
    if (name, mode) not in _GRIDS:
        g = orc.Scene(*lm.get(name)).voxelize(16, mode=mode, algo=orc.ALGO_BRUTE)
        g.setflags(write=False)
        _GRIDS[name, mode] = g
    return _GRIDS[name, mode]


@pytest.mark.parametrize("name", WALK_CASES)
def test_walks_equal_the_brute_force_oracle(dxv, orc, name):
    vb, ib = lm.get(name)
    v = dxv.Voxelizer(0)
    try:
        for lists, wide in ((0, 2), (0, 1), (0, 0), (1, 2), (2, 2)):
            v.set_option("lists", lists)
            v.set_option("wide", wide)
            v.InitDynamic(vb, ib)
            for mode in (0, 1):
                for launch in range(2):                      # (lists 1: the second launch of a scene is the one through the lists)
                    v.Voxelize(16, mode)
                    assert np.array_equal(v.Grid(), oracle_grid(orc, name, mode)), (name, "lists", lists, "wide", wide, "mode", mode, "launch", launch)
    finally:
        v.close()


def round_up_column(n):
    return next(c for c in (8, 12, 16, 20, 24, 32, 48, 64) if n <= c)


@pytest.mark.parametrize("name,height,wide_walk", [("comb-7", 38, True), ("comb-8", 39, False), ("comb-8-soup", 39, False)])
def test_tall_trees_straddle_the_wide_walks_limit(dxv, orc, name, height, wide_walk):
    """dxv_frames.hip, `Stack policy`: the wide walk pushes up to three entries per two binary levels and keeps four more slots,
    3 * ceil(h / 2) + 5, and is used while that fits the largest column of 64; the binary walk needs h + 3.  h = 38: 3 * 19 + 5 = 62,
    wide, safe column 64.  h = 39: 3 * 20 + 5 = 65 > 64, binary, 42 entries, safe column 48.

    stats()["stack_entries"] is the column the launch ran with, not the safe one: a launch starts with min(h + 3, stack0 = 20) entries
    (dxv_ctx.h, initial_stack) and grows towards the safe column only when the redo pass's list of 65 536 rays fills, which a 16^3
    launch cannot do.  So the starting column, 20, is what is asserted, and that it does not exceed the safe one.

    Nor does a high tree make a deep walk: the combs' triangles are 2^-12 wide, and the host's walk of them at 16^3 never holds more
    than 3 entries (2 at b = 7; histogram of the greatest depth per ray at b = 8: 3851, 195, 46, 4), so 8 entries hold every ray and
    the redo pass has nothing to do there: on the combs the 8-entry launch is held to the same grid only.  The redo pass on a tree of
    height 39 is held on comb-8-soup, whose host walk reaches depth 12 (tests/test_lbvh_rule.py asserts it): more than any 8-entry
    column holds, so redo_rays > 0 there, and the grid is the same."""
    vb, ib = lm.get(name)
    safe = round_up_column(3 * ((height + 1) // 2) + 5) if wide_walk else round_up_column(height + 3)
    assert (3 * ((height + 1) // 2) + 5 <= 64) == wide_walk and safe == (64 if wide_walk else 48)
    v = dxv.Voxelizer(0)
    try:
        v.set_option("lists", 0)
        v.InitDynamic(vb, ib)
        assert v.stats()["tree_height"] == height
        want = oracle_grid(orc, name, 0)
        v.Voxelize(16)
        assert np.array_equal(v.Grid(), want)
        assert v.stats()["stack_entries"] == round_up_column(min(height + 3, 20)) <= safe
        v.set_option("stack", 8)
        v.Voxelize(16)
        st = v.stats()
        assert st["stack_entries"] == 8
        assert np.array_equal(v.Grid(), want), "the 8-entry launch and its redo pass give another grid"
        if name == "comb-8-soup":
            assert st["redo_rays"] > 0, "no ray ran out of 8 entries on a walk that needs 12"
        v.set_option("stack", 64)                            # a column that holds either walk whole: no ray is redone
        v.Voxelize(16)
        st = v.stats()
        assert st["stack_entries"] == 64 and st["redo_rays"] == 0, st
        assert np.array_equal(v.Grid(), want)
    finally:
        v.close()


@pytest.mark.parametrize("name", ["comb-8", "copies-1025"])
def test_mesh_distance_over_a_tall_tree_and_over_equal_distances(dxv, name):
    """comb-8: a tree of height 39 under the nearest-triangle walk's column; copies-1025: every triangle at the same distance from every
    voxel, the smallest index must win"""
    vb, ib = lm.get(name)
    v = dxv.Voxelizer(0)
    try:
        v.InitDynamic(vb, ib)
        v.Voxelize(8)
        want, tri = mr.field_of_mesh(vb, ib, 8, v.Grid(), mr.VOXELS_F32, 0)
        got = v.MeshDistanceField(dxv.MDIST_VOXELS_F32, 0, True)
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), name
        assert np.array_equal(v.MeshDistanceTriangles(), tri), name
        if name.startswith("copies"):
            assert not tri.any()
    finally:
        v.close()
