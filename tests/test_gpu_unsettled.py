"""Every operator of a frame's grid behind every operator that is still unsettled (tests/unsettled_cases.py: the grid, the leaders, the followers,
the wanted results and the conditions that make these comparisons tests; tests/test_unsettled_cases.py runs those on the CPU).  A leader -- a fill,
a thin, a geodesic, an access at one round per batch, an expansion from a caller's tree -- is enqueued with sync=False, a follower right behind
it with no synchronisation of any kind in between, then the frame is synchronised once: the grid, the follower's product with its tables,
histograms and tallies, and the leader's own report are those of the host libraries on the grid the leader leaves, byte for byte.  What exists
only on the host side of the library -- that every entry finishes what is unsettled before it reads the grid or the frame's state
(csrc/dxv_frames.hip: settle_frame_launch; csrc/dxv_products.hip: begin_operator, begin_seeded, settle_batched) -- runs here.

The matrix is 5 leaders x 56 followers = 280 cells: the 28 followers of unsettled_cases.PLAIN_FOLLOWERS, and each of them once more with a
trim as the synchronisation and the same follower again in the scratch the trim gave back.  Beside it: the wide side's diagonal, a chain four
deep, the batch size changed behind the leader's back, three frames in flight, and products made before an editing leader and asked for after it.
No number here is a tolerance or a time; the one threshold, three rounds, is unsettled_cases.MIN_ROUNDS and is argued there."""
import re

import numpy as np
import pytest

import unsettled_cases as uc
from raycast_restated import write_grid
from test_gpu_octree import as_device_words

pytestmark = pytest.mark.gpu

CELLS = [(name, follower) for name in uc.LEADERS for follower in uc.FOLLOWERS]
assert len(CELLS) == len(set(CELLS)) == uc.CELLS == 280 and {f for _, f in CELLS} == set(uc.FOLLOWERS)

GEO_TALLY = ("seeds_used", "reached", "unreached", "farthest", "farthest_voxel")
ACC_TALLY = ("seeds_used", "reached", "unreached", "widest", "widest_voxel")
STALE = {"geodesic": "dxv_geodesic_info: frame {} was launched or edited again since its geodesic map was made: the map is stale",
         "access": "dxv_access_info: frame {} was launched or edited again since its access map was made: maps and histograms are stale"}
# dxv_grid_count, dxv_grid_download_packed and dxv_grid_download finish what may still change the grid (csrc/dxv_api.hip: finish_launch); a flood,
# which only reads it, they leave to the frame's next synchronisation
GRID_READERS = ("count", "bits", "grid")
SPARE_FRAME = 2                                                         # where the render follower's wanted image is made


@pytest.fixture(scope="module")
def dxv(dxvlib):
    import dxrvoxelizer_amd
    return dxrvoxelizer_amd


@pytest.fixture(scope="module")
def writer(dxv, bunny):
    """the one Voxelizer, on the bunny, whose frames every grid of this file is written into: every leader at one round per batch"""
    vb, ib, _ = bunny
    v = dxv.Voxelizer(0)
    try:
        v.InitFromArrays(vb, ib)
        yield v
    finally:
        v.close()


@pytest.fixture
def v(writer):
    """... with the options set for a test and put back behind it, and frame 0 selected"""
    try:
        for key in uc.ROUNDS_OPTION.values():
            writer.set_option(key, 1)
        writer.set_option("events", 1)
        writer.SetFrame(0)
        yield writer
    finally:
        for key in uc.ROUNDS_OPTION.values():
            writer.set_option(key, 0)
        writer.SetFrame(0)
        writer.Sync()


def load(v, g, frame=0):
    """a fresh launch of the frame at g's side -- every product of the frame is stale, nothing is unsettled -- and g in its grid"""
    v.Voxelize(g.shape[0], frameIndex=frame)
    write_grid(v, np.array(g))                                          # (a copy: the wanted results are read-only, and torch wants to be able to write)


# ---- what is made ready before the leader: device memory a call is handed, so that nothing synchronises between leader and follower -----------
def ready_leader(v, lead):
    return {"tree": as_device_words(lead.args["nodes"])} if lead.name == "expand" else {}


def ready_follower(v, what, w):
    import torch
    state = {}
    if what == "expand a tree":
        state["tree"] = as_device_words(w["args"]["nodes"])
    if what == "render":
        eye, view_proj = uc.camera_of(w["grid"].shape[0])
        state["target"] = torch.zeros((uc.VIEW[1], uc.VIEW[0], 4), dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        v.UpdateFrame(v._frame, eye, view_proj, uc.VIEW[0], uc.VIEW[1])
    return state


def enqueue_leader(v, dxv, lead, state):
    if lead.name == "fill":
        assert v.Fill(sync=False) is True
    elif lead.name == "thin":
        assert v.Thin(dxv.THIN_CURVE, sync=False) is True
    elif lead.name == "geodesic":
        assert v.Geodesic(lead.args["of"], dxv.GEO_CHAMFER, lead.args["seeds"], sync=False) is True
    elif lead.name == "access":
        assert v.Access(lead.args["of"], 6, uc.ACCESS_CAP, lead.args["seeds"], True, sync=False) is True
    else:
        assert v.OctreeExpand(state["tree"], levels=lead.args["levels"], sync=False) is True


def follower_steps(v, dxv, what, w, state):
    """the follower's call or chain of calls, one callable each, every one with sync=False; the three readers of the grid block by their nature"""
    bits = uc.sr.axis_bits(uc.SIGHT_FILL_AXIS)
    chains = {
        "distance i32": [lambda: v.DistanceField(dxv.DIST_SQ_I32, sync=False)],
        "distance f32": [lambda: v.DistanceField(dxv.DIST_F32, sync=False)],
        "mesh distance": [lambda: v.MeshDistanceField(dxv.MDIST_VOXELS_F32, 0, True, sync=False)],
        "isosurface of the grid field": [lambda: v.DistanceField(dxv.DIST_F32, sync=False), lambda: v.Isosurface(dxv.ISO_GRID_DISTANCE, uc.ISO_GRID, dxv.ISO_SPACE_VOXELS, sync=False)],
        "isosurface of the mesh field": [lambda: v.MeshDistanceField(dxv.MDIST_VOXELS_F32, 0, False, sync=False), lambda: v.Isosurface(dxv.ISO_MESH_DISTANCE, uc.ISO_MESH, dxv.ISO_SPACE_VOXELS, sync=False)],
        "octree": [lambda: v.Octree(sync=False)],
        "expand own tree": [lambda: v.Octree(sync=False), lambda: v.OctreeExpand(sync=False)],
        "expand a tree": [lambda: v.OctreeExpand(state["tree"], levels=w["args"]["levels"], sync=False)],
        "components": [lambda: v.Components(dxv.COMP_SOLID, 6, sync=False)],
        "measure": [lambda: v.Components(dxv.COMP_EMPTY, 6, sync=False), lambda: v.Measure(sync=False)],
        "select": [lambda: v.Components(dxv.COMP_SOLID, 6, sync=False), lambda: v.SelectComponents(dxv.SELECT_MIN_VOXELS, 2, sync=False)],
        "thickness": [lambda: v.Thickness(dxv.COMP_SOLID, uc.THICK_CAP, sync=False)],
        "partition": [lambda: v.Partition(dxv.COMP_SOLID, uc.PART_CAP, True, sync=False)],
        "skeleton": [lambda: v.Skeleton(sync=False)],
        "prune": [lambda: v.Skeleton(sync=False), lambda: v.SkeletonPrune(uc.PRUNE_LEN, sync=False)],
        "geodesic": [lambda: v.Geodesic(dxv.COMP_EMPTY, dxv.GEO_FACES, "border", sync=False)],
        "geodesic path": [lambda: v.Geodesic(dxv.COMP_EMPTY, dxv.GEO_FACES, "border", sync=False), lambda: state.update(path=v.GeodesicPath(w["args"]["target"]))],
        "access": [lambda: v.Access(dxv.COMP_EMPTY, 26, uc.ACCESS_CAP, "border", True, sync=False)],
        "sight": [lambda: v.Sight(dxv.COMP_EMPTY, dxv.SIGHT_ALL, sync=False)],
        "sight fill": [lambda: v.Sight(dxv.COMP_SOLID, dxv.SIGHT_ALL, sync=False), lambda: v.SightFill(bits, sync=False)],
        "fill": [lambda: v.Fill(sync=False)],
        "dilate": [lambda: v.Morph(dxv.MORPH_DILATE, 1, sync=False)],
        "erode": [lambda: v.Morph(dxv.MORPH_ERODE, 1, sync=False)],
        "thin": [lambda: v.Thin(dxv.THIN_KERNEL, sync=False)],
        "render": [lambda: v.RenderAsync(state["target"])],
        "count": [lambda: state.update(count=v.CountSolid())],
        "bits": [lambda: state.update(bits=v.GridBits())],
        "grid": [lambda: state.update(grid=v.Grid())],
    }
    assert chains.keys() == set(uc.PLAIN_FOLLOWERS)
    return chains[what]


def enqueue_follower(v, dxv, what, w, state, behind_the_first=None):
    """... behind_the_first(): called as soon as the first of them has returned, the one that stands right behind the leader"""
    for k, step in enumerate(follower_steps(v, dxv, what, w, state)):
        step()
        if k == 0 and behind_the_first:
            behind_the_first()


def read_follower(v, what, state):
    """what the follower made, once the frame has been synchronised: the keys of its wanted result but the grid"""
    if what in ("distance i32", "distance f32"):
        return {"field": v.Distance()}
    if what == "mesh distance":
        return {"field": v.MeshDistance(), "triangles": v.MeshDistanceTriangles()}
    if what.startswith("isosurface"):
        vb, ib = v.IsosurfaceMesh()
        return {"field": v.Distance() if "grid" in what else v.MeshDistance(), "vb": vb, "ib": ib}
    if what == "octree":
        nodes, first = v.OctreeNodes()
        return {"nodes": nodes, "level_first": first}
    if what == "components":
        return {"labels": v.ComponentLabels(), "table": v.ComponentTable()}
    if what == "measure":
        return {"labels": v.ComponentLabels(), "table": v.ComponentTable(), "measure": v.MeasureTable()}
    if what == "select":
        return {"select_info": v.select_info()}
    if what == "thickness":
        return {"field": v.ThicknessField(), "histogram": v.ThicknessHistogram(), "info": v.ThicknessInfo()[1:]}
    if what == "partition":
        return {"labels": v.PartitionLabels(), "table": v.PartitionTable(), "throats": v.PartitionThroats(), "info": v.PartitionInfo()[1:]}
    if what == "skeleton":
        info = v.SkeletonInfo()
        return {"labels": v.SkeletonLabels(), "nodes": v.SkeletonNodes(), "branches": v.SkeletonBranches(),
                "info": (info["nodes"], info["branches"], info["end_voxels"], info["curve_voxels"], info["junction_voxels"])}
    if what == "prune":
        return {"prune_info": v.SkeletonPruneInfo()}
    if what in ("geodesic", "geodesic path"):
        info = v.GeodesicInfo()
        out = {"field": v.GeodesicField(), "tally": {k: info[k] for k in GEO_TALLY}}
        if what == "geodesic path":
            out["path"] = state["path"]
        return out
    if what == "access":
        info = v.AccessInfo()
        return {"A": v.AccessField(), "I": v.IntrusionField(), "hist_a": v.AccessHistogram(), "hist_i": v.IntrusionHistogram(), "tally": {k: info[k] for k in ACC_TALLY}}
    if what == "sight":
        return {"field": v.SightField(), "tally": v.SightTally()}
    if what == "fill":
        return {"rounds": v.fill_info()[1]}
    if what in ("dilate", "erode"):
        return {"morph_info": v.morph_info()[1:]}
    if what == "thin":
        return {"thin_info": v.thin_info()[1:]}
    if what == "render":
        return {"image": state["target"].cpu().numpy()}
    if what in ("count", "bits"):
        return {what: state[what]}
    return {}


def same_tally(got, want):
    return got["members"] == want["members"] and all(np.array_equal(np.asarray(got[k], np.uint64), np.asarray(want[k], np.uint64)) for k in ("seen", "neither", "count"))


def check_follower(v, what, w, state, cell):
    """the grid and the follower's product against its wanted result w: byte equality, no tolerance"""
    got = read_follower(v, what, state)
    wanted = {k: x for k, x in uc.observed(w).items() if k != "grid"}
    if what == "render":                                                # (with dxv_render of the wanted grid in a frame of its own: the same kernel, the same constants)
        frame = v._frame
        load(v, w["grid"], SPARE_FRAME)
        eye, view_proj = uc.camera_of(w["grid"].shape[0])
        wanted = {"image": v.Render(eye, view_proj, uc.VIEW[0], uc.VIEW[1])}
        v.SetFrame(frame)
        assert len(np.unique(wanted["image"].reshape(-1, 4), axis=0)) >= 3, cell
    assert got.keys() == wanted.keys(), (cell, sorted(got), sorted(wanted))
    for k in wanted:
        if what == "sight" and k == "tally":
            assert same_tally(got[k], wanted[k]), (cell, k, got[k], wanted[k])
        else:
            assert uc.same(got[k], wanted[k]), (cell, k)
    if what == "grid":
        assert np.array_equal(state["grid"], w["grid"]), cell
    grid = v.Grid()
    assert grid.dtype == np.uint8 and np.array_equal(grid, w["grid"]), (cell, int(np.count_nonzero(grid != w["grid"])))


def check_leader(v, dxv, lead, what, edited, cell):
    """the leader's own report behind the chain, as of the same leader run alone and synchronously.  what: the follower; edited: the grid it left"""
    frame = v._frame
    if lead.name == "fill" and what != "fill":
        ms, rounds = v.fill_info()
        assert rounds == lead.report["rounds"] and ms > 0.0, (cell, ms, rounds)
    elif lead.name == "thin" and what != "thin":
        info = v.thin_info()
        assert info[1:] == lead.report["thin_info"] and info[0] > 0.0, (cell, info)
    elif lead.name in ("geodesic", "access") and what not in uc.REPLACES[lead.name]:
        reads = v.GeodesicInfo if lead.name == "geodesic" else v.AccessInfo
        if what in uc.EDITORS:
            # the follower rewrote the grid: the leader was finished in front of it, its map is refused, and the same leader again is the host's on the edited grid
            with pytest.raises(dxv.DxvError, match="^" + re.escape(STALE[lead.name].format(frame)) + "$"):
                reads()
            report, seeds = uc.flood_again(lead.name, edited)
            if lead.name == "geodesic":
                got = {"field": v.Geodesic(uc.SOLID, dxv.GEO_CHAMFER, seeds)}
            else:
                A, I = v.Access(uc.SOLID, 6, uc.ACCESS_CAP, seeds)
                got = {"A": A, "I": I, "hist_a": v.AccessHistogram(), "hist_i": v.IntrusionHistogram()}
            info = reads()
            assert np.array_equal(v.Grid(), edited), cell
        else:
            # the follower only read: map, histograms and tally are still current
            report = lead.report
            info = reads()
            if lead.name == "geodesic":
                got = {"field": v.GeodesicField()}
            else:
                got = {"A": v.AccessField(), "I": v.IntrusionField(), "hist_a": v.AccessHistogram(), "hist_i": v.IntrusionHistogram()}
            # at one round per batch the leader was unsettled when the follower came: unsettled_cases.leader has the argument for D + 1 rounds
            assert info["rounds"] >= uc.MIN_ROUNDS, (cell, info)
        assert info["ms"] > 0.0, (cell, info)
        got["tally"] = {k: info[k] for k in (GEO_TALLY if lead.name == "geodesic" else ACC_TALLY)}
        assert got.keys() == report.keys() and not uc.differing(got, report), (cell, uc.differing(got, report), got["tally"], report["tally"])


def check_settled(v, dxv, lead, what, cell):
    """as soon as the follower's first call has returned -- nothing has synchronised the frame -- the leader is finished (include/dxv.h: "a pending
    fill, thin, expansion, geodesic or access of the frame is settled first"): its report is already the whole one.  what: the follower"""
    if lead.name == "fill" and what != "fill":
        assert v.fill_info()[1] == lead.report["rounds"], (cell, v.fill_info())
    elif lead.name == "thin" and what != "thin":
        assert v.thin_info()[1:] == lead.report["thin_info"], (cell, v.thin_info())
    elif lead.name in ("geodesic", "access") and what not in uc.REPLACES[lead.name] and what not in GRID_READERS:
        reads = v.GeodesicInfo if lead.name == "geodesic" else v.AccessInfo
        if what in uc.EDITORS and len(follower_steps(v, dxv, what, None, None)) == 1:
            with pytest.raises(dxv.DxvError, match="^" + re.escape(STALE[lead.name].format(v._frame)) + "$"):
                reads()
        else:                                                           # (a chain's first call only reads)
            info = reads()
            tally = {k: info[k] for k in (GEO_TALLY if lead.name == "geodesic" else ACC_TALLY)}
            assert tally == lead.report["tally"] and info["rounds"] >= uc.MIN_ROUNDS, (cell, info)


def run_cell(v, dxv, name, follower, g, between=None):
    """one cell of the matrix on the selected frame: write the grid, the leader, the follower, one synchronisation, every comparison"""
    lead, w, again = uc.pair(name, follower, g)
    what, cell = uc.plain(follower), (name, follower, g.shape[0])
    load(v, g, v._frame)
    state = {**ready_leader(v, lead), "follower": ready_follower(v, what, w)}
    enqueue_leader(v, dxv, lead, state)
    if between:
        between()
    enqueue_follower(v, dxv, what, w, state["follower"], lambda: check_settled(v, dxv, lead, what, cell))     # (no synchronisation of any kind since the leader)
    if again is None:
        v.Sync()
    else:
        v.trim()                                                        # (synchronises every frame and gives every operator's scratch back)
    check_follower(v, what, w, state["follower"], cell)
    check_leader(v, dxv, lead, what, w["grid"], cell)
    if again is not None:
        # the same follower once more, on the grid the first one left, in scratch that has to be made again
        second = ready_follower(v, what, again)
        enqueue_follower(v, dxv, what, again, second)
        v.Sync()
        check_follower(v, what, again, second, cell + ("again",))


# ---- the matrix -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name, follower", CELLS, ids=[f"{name} - {follower}" for name, follower in CELLS])
def test_a_follower_behind_an_unsettled_leader(v, dxv, name, follower):
    """280 cells: every one of the five leaders with every one of the 56 followers, at side 22"""
    assert len(CELLS) == 280
    run_cell(v, dxv, name, follower, uc.grid(uc.SIDE))


# ---- beside it ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", uc.LEADERS)
def test_the_diagonal_at_the_wide_side(v, dxv, name):
    """rows of two words, a second trip of the tallies' loops: an editor, a batched follower and a map behind every leader"""
    g = uc.grid(uc.WIDE_SIDE)
    for follower in uc.DIAGONAL[name]:
        run_cell(v, dxv, name, follower, g)


def test_four_deep(v, dxv):
    """Fill -> Thin -> Geodesic -> Access -> Sight, nothing synchronised in between, every batched one at one round per batch"""
    g = uc.grid(uc.SIDE)
    fill, thin, geodesic, access, sight = uc.four_deep(g)
    load(v, g)
    enqueue_leader(v, dxv, fill, {})
    enqueue_leader(v, dxv, thin, {})
    enqueue_leader(v, dxv, geodesic, {})
    enqueue_leader(v, dxv, access, {})
    assert v.Sight(dxv.COMP_EMPTY, dxv.SIGHT_ALL, sync=False) is True
    for lead in (fill, thin, geodesic, access):                         # every one of them was finished by the call behind it
        check_settled(v, dxv, lead, "sight", "four deep")
    v.Sync()
    assert np.array_equal(v.Grid(), thin.after)
    ms, rounds = v.fill_info()
    assert rounds == fill.report["rounds"] >= uc.MIN_ROUNDS and ms > 0.0
    info = v.thin_info()
    assert info[1:] == thin.report["thin_info"] and info[1] >= uc.MIN_ROUNDS and info[0] > 0.0
    check_leader(v, dxv, geodesic, "sight", thin.after, "four deep")
    check_leader(v, dxv, access, "sight", thin.after, "four deep")
    assert uc.same(v.SightField(), sight["field"]) and same_tally(v.SightTally(), sight["tally"])
    assert np.array_equal(v.Grid(), thin.after)


@pytest.mark.parametrize("name", uc.BATCHED_LEADERS)
def test_the_batch_size_belongs_to_the_call(v, dxv, name):
    """the leader's rounds option set to 4 and then to 0 between its _async and the follower: the batches behind the first one are the call's,
    of one round (include/dxv.h: "as it stood at the operator's _async"), and results and reports are as before"""
    key = uc.ROUNDS_OPTION[name]

    def between():
        v.set_option(key, 4)
        v.set_option(key, 0)
    for follower in ("sight", "erode"):
        v.set_option(key, 1)
        run_cell(v, dxv, name, follower, uc.grid(uc.SIDE), between)


def test_three_frames_each_with_its_own_leader_unsettled(v, dxv):
    """frames 0, 1 and 2 at sides 22, 18 and 24: a leader on each, then a follower on each while the other two are still unsettled, SyncAll"""
    cases = [(frame, uc.grid(N)) + uc.pair(name, follower, uc.grid(N))[:2] + (follower,) for frame, (N, name, follower) in enumerate(uc.FRAMES)]
    for frame, g, lead, w, follower in cases:
        load(v, g, frame)
    states = {}
    for frame, g, lead, w, follower in cases:
        v.SetFrame(frame)
        states[frame] = {**ready_leader(v, lead), "follower": ready_follower(v, follower, w)}
    for frame, g, lead, w, follower in cases:
        v.SetFrame(frame)
        enqueue_leader(v, dxv, lead, states[frame])
    for frame, g, lead, w, follower in cases:                           # (the other two frames stay unsettled)
        v.SetFrame(frame)
        enqueue_follower(v, dxv, follower, w, states[frame]["follower"], lambda: check_settled(v, dxv, lead, follower, (frame, lead.name, follower)))
    v.SyncAll()
    pointers = []
    for frame, g, lead, w, follower in cases:
        v.SetFrame(frame)
        assert v.stats()["grid_dim"] == g.shape[0]
        check_follower(v, follower, w, states[frame]["follower"], (frame, lead.name, follower))
        check_leader(v, dxv, lead, follower, w["grid"], (frame, lead.name, follower))
        pointers += [v.grid_device_ptr(writable=False), v.thickness_device_ptr()]
    assert len(set(pointers)) == 6 and all(pointers)                   # three grids and three maps, each frame's own


@pytest.mark.parametrize("name", uc.EDITING_LEADERS)
def test_a_product_made_before_an_editing_leader_is_refused_behind_it(v, dxv, name):
    """a field, a labelling, a skeleton, a tree and a line-of-sight map made of the grid, then the leader with sync=False: every consumer of
    them is refused with its stale message and launches nothing, and the leader settles to the host's grid at the next Sync"""
    lib, ctx = v._lib, v._ctx
    g = uc.grid(uc.SIDE)
    lead = uc.leader(name, g)
    load(v, g)
    v.DistanceField(dxv.DIST_F32)
    v.MeshDistanceField(dxv.MDIST_VOXELS_F32)
    v.Components(dxv.COMP_SOLID, 6)
    v.Skeleton()
    v.Octree()
    v.Sight(dxv.COMP_SOLID, dxv.SIGHT_ALL)
    state = ready_leader(v, lead)
    enqueue_leader(v, dxv, lead, state)
    refused = [(lambda: lib.dxv_isosurface_async(ctx, dxv.ISO_GRID_DISTANCE, uc.ISO_GRID, 0), "dxv_isosurface: frame 0 was launched or filled again since its distance field was made: the field is stale"),
               (lambda: lib.dxv_isosurface_async(ctx, dxv.ISO_MESH_DISTANCE, uc.ISO_MESH, 0), "dxv_isosurface: frame 0 was launched or filled again since its mesh distance field was made: the field is stale"),
               (lambda: lib.dxv_measure_async(ctx), "dxv_measure: frame 0 was launched, filled, expanded or selected again since its components were labelled: labels and table are stale"),
               (lambda: lib.dxv_components_select_async(ctx, dxv.SELECT_MIN_VOXELS, 2),
                "dxv_components_select: frame 0 was launched, filled, expanded or selected again since its components were labelled: labels and table are stale"),
               (lambda: lib.dxv_skeleton_prune_async(ctx, uc.PRUNE_LEN), "dxv_skeleton_prune: frame 0 was launched or edited again since its skeleton was made: labels and tables are stale"),
               (lambda: lib.dxv_octree_expand_async(ctx, None, 0, 0), "dxv_octree_expand: frame 0 was launched, filled or expanded again since its octree was made: the tree is stale"),
               (lambda: lib.dxv_sight_fill_async(ctx, uc.sr.axis_bits(uc.SIGHT_FILL_AXIS)),
                "dxv_sight_fill: frame 0 was launched or edited again since its line-of-sight map was made: map and tally are stale")]
    for call, text in refused:
        assert call() == 1 and lib.dxv_last_error(ctx).decode() == text, (name, text, lib.dxv_last_error(ctx).decode())
    v.Sync()
    assert np.array_equal(v.Grid(), lead.after), name                  # nothing but the leader touched the grid
    check_leader(v, dxv, lead, "grid", lead.after, (name, "stale products"))
