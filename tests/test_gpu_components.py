"""Connected components on the GPU (include/dxv.h: dxv_components*): the device's labels and table equal the numpy restatement
(tests/components_restated.py) of the grid they were made from -- array_equal, no tolerance, both kinds and both connectivities -- for
arbitrary grids written through the frame's grid pointer, for meshes in every mode, for large grids against committed hashes
(tests/golden/components.json, tests/gen_components_fixtures.py); SelectComponents edits the grid as the restatement does and, for the empty
space under 6 from the border, as the fill does; three frames label side by side; labels go stale when their grid changes; and the calls
refuse what they must."""
import ctypes as C
import hashlib
import json
import os

import numpy as np
import pytest

import components_restated as cr
import fill_restated as fr
from conftest import GOLD, load_mesh
from raycast_restated import write_grid

pytestmark = pytest.mark.gpu

KINDS = (cr.SOLID, cr.EMPTY)
CONNECTIVITIES = (6, 26)
_RESTATED = {}


@pytest.fixture(scope="module")
def dxv(dxvlib):
    import dxrvoxelizer_amd
    return dxrvoxelizer_amd


@pytest.fixture(scope="module")
def writer(dxv, bunny):
    vb, ib, _ = bunny
    v = dxv.Voxelizer(0)
    v.InitFromArrays(vb, ib)
    yield v
    v.close()


def restated(key, g, of, conn):
    """the restatement of grid g, computed once per (key, kind, connectivity) and left unchanged"""
    k = (key, of, conn)
    if k not in _RESTATED:
        labels, table = cr.label(g, of, conn)
        labels.setflags(write=False)
        table.setflags(write=False)
        _RESTATED[k] = (labels, table)
    return _RESTATED[k]


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def check(v, key, g, of, conn):
    """the selected frame's labelling against the restatement of grid g; returns (labels, table)"""
    want, wtable = restated(key, g, of, conn)
    labels, table = v.Components(of, conn)
    N = g.shape[0]
    assert labels.dtype == np.uint32 and labels.shape == (N, N, N) and np.array_equal(labels, want), (key, of, conn)
    assert table.dtype == cr.RECORD and np.array_equal(table, wtable), (key, of, conn)
    assert v.components_info() == (len(wtable), of, conn), key
    assert v._lib.dxv_components_labels_bytes(v._ctx) == 4 * N ** 3 and v._lib.dxv_components_table_bytes(v._ctx) == 24 * len(wtable), key
    lp, tp = v.component_device_ptrs()
    assert lp and bool(tp) == bool(len(wtable)), key
    return labels, table


GRID_NAMES = ("random 0.2", "random 0.3", "random 0.6", "random 0.68", "all zero", "all 0xFF", "checkerboard", "one voxel")


def grid_of(N, what):
    if what.startswith("random"):
        return fr.random_walls(N, float(what.split()[1]), 1000 + N, bytes_other_than_one=True)
    return {"all zero": lambda: np.zeros((N, N, N), np.uint8), "all 0xFF": lambda: np.full((N, N, N), 0xFF, np.uint8),
            "checkerboard": lambda: cr.checkerboard(N), "one voxel": lambda: cr.one_voxel(N)}[what]()


def fill_equivalence(v, g, what):
    """Components(EMPTY, 6); Select(BORDER) leaves the fill's solid: the restatement's and the device's own"""
    write_grid(v, g)
    v.Components(cr.EMPTY, 6)
    v.SelectComponents(cr.BORDER)
    got = v.Grid()
    assert np.array_equal(got != 0, fr.fill(g) != 0), what
    assert np.array_equal(got[g != 0], g[g != 0]), what                 # (the walls keep their bytes)
    write_grid(v, g)
    v.Fill()
    assert np.array_equal(got != 0, v.Grid() != 0), what


@pytest.mark.parametrize("what", GRID_NAMES)
@pytest.mark.parametrize("N", [2, 64, 66, 96])          # 2: all border; 66: rows of one word and two bits, the N & 7 pack path; 96: a word and a half
def test_written_grids_equal_restatement(dxv, writer, N, what):
    v = writer
    v.Voxelize(N)
    g = grid_of(N, what)
    key = f"{what} {N}"
    for of in KINDS:
        for conn in CONNECTIVITIES:
            write_grid(v, g)
            labels, table = check(v, key, g, of, conn)
            K = len(table)
            if what.startswith("random") and N > 2:
                assert K > 1 or conn == 26, (key, of, conn, K)
            if what == "all zero":
                assert K == (0 if of == cr.SOLID else 1)
            if what == "all 0xFF":
                assert K == (1 if of == cr.SOLID else 0)
                if K:
                    assert table[0]["voxels"] == N ** 3 and table[0]["flags"] == 1 and table[0]["hi"].tolist() == [N - 1] * 3
            if what == "checkerboard" and of == cr.SOLID:
                assert K == (N ** 3 // 2 if conn == 6 else 1)
            if what == "one voxel" and of == cr.SOLID:
                assert K == 1 and table[0]["voxels"] == 1
    fill_equivalence(v, g, key)
    assert v.components_ms() > 0.0


def test_random_grids_cannot_pass_vacuously(dxv, writer):
    v = writer
    v.Voxelize(64)
    g = fr.random_walls(64, 0.68, 1064, bytes_other_than_one=True)
    assert len(restated("random 0.68 64", g, cr.EMPTY, 6)[1]) > 5000     # thousands of pores
    g = fr.random_walls(64, 0.3, 1064, bytes_other_than_one=True)
    assert len(restated("random 0.3 64", g, cr.SOLID, 6)[1]) > 5000 and 1 < len(restated("random 0.3 64", g, cr.SOLID, 26)[1]) < 1000


def test_the_baffle_maze_is_one_long_component(dxv, writer):
    v = writer
    v.Voxelize(32)
    g = fr.maze(32)                                                     # one serpentine: the deepest parent chains
    for of in KINDS:
        for conn in CONNECTIVITIES:
            write_grid(v, g)
            _, table = check(v, "maze 32", g, of, conn)
            assert len(table) == 1
    fill_equivalence(v, g, "maze 32")


@pytest.mark.parametrize("name", ["bunny", "dragon", "turingbowl"])
def test_mesh_grids_equal_restatement(dxv, name):
    vb, ib, _ = load_mesh(name)
    v = dxv.Voxelizer(0)
    try:
        v.InitFromArrays(vb, ib)
        for mode in (0, 1, 2, 3):
            v.Voxelize(64, mode)
            g = v.Grid()
            assert g.any()
            for of in KINDS:
                for conn in CONNECTIVITIES:
                    _, table = check(v, f"{name} mode {mode}", g, of, conn)
                    vox = table["voxels"]
                    print(f"{name} 64 mode {mode} of {of} conn {conn}: K {len(table)}, largest {int(vox.max()) if len(vox) else 0}, "
                          f"singletons {int((vox == 1).sum())}, {v.components_ms():.3f} ms")
                    assert len(table) >= 1
            fill_equivalence(v, g, f"{name} mode {mode}")
    finally:
        v.close()


# ---- select -------------------------------------------------------------------------------------------------------------------------------
def check_select(v, key, g):
    for of in KINDS:
        for conn in CONNECTIVITIES:
            labels, table = restated(key, g, of, conn)
            for rule, arg in ((cr.LARGEST, 0), (cr.MIN_VOXELS, 3), (cr.MIN_VOXELS, 40), (cr.BORDER, 0)):
                want, counts = cr.select(g, labels, table, of, rule, arg)
                write_grid(v, g)
                v.Components(of, conn)
                assert v.SelectComponents(rule, arg) is True
                got = v.Grid()
                assert np.array_equal(got, want), (key, of, conn, rule, arg)
                assert v.select_info() == counts, (key, of, conn, rule, arg, v.select_info(), counts)
                assert v.CountSolid() == int(np.count_nonzero(want)), (key, of, conn, rule)
                with pytest.raises(v_error(v), match="stale"):
                    v.components_info()


def v_error(v):
    import dxrvoxelizer_amd
    return dxrvoxelizer_amd.DxvError


def test_select_on_a_random_grid_and_a_mesh_grid(dxv, writer):
    v = writer
    v.Voxelize(64)
    g = fr.random_walls(64, 0.3, 1064, bytes_other_than_one=True)
    check_select(v, "random 0.3 64", g)
    v.Voxelize(64, dxv.MODE_SURFACE)
    g = v.Grid()
    g[3, 3, 3] = 0x40                                                   # a floater and a pore of one voxel each
    g[g.shape[0] // 2, g.shape[0] // 2, 3] = 7
    check_select(v, "bunny surface 64 with a floater", g)
    write_grid(v, g)
    v.Components(cr.SOLID, 26)
    v.SelectComponents(cr.LARGEST, sync=False)                          # enqueued only: the counters come with the frame's Sync
    v.Sync()
    kept, dropped, changed = v.select_info()
    assert kept == 1 and dropped >= 1 and changed >= 1 and v.Grid()[3, 3, 3] == 0


# ---- large grids --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", ["bunny/256", "torus1m/512"])
def test_large_grids_equal_committed_hashes(dxv, key):
    from dxrvoxelizer_amd import meshes
    with open(os.path.join(GOLD, "components.json")) as fh:
        want = json.load(fh)[key]
    name, N = key.split("/")
    vb, ib = meshes.torus() if name == "torus1m" else load_mesh(name)[:2]
    v = dxv.Voxelizer(0)
    try:
        v.InitFromArrays(vb, ib)
        v.Voxelize(int(N), dxv.MODE_REFERENCE)
        assert sha(v.Grid()) == want["grid_sha256"], f"{key}: the grid is not the one the fixture was made from"
        for of, kind in ((cr.SOLID, "solid"), (cr.EMPTY, "empty")):
            for conn in CONNECTIVITIES:
                row = want[f"{kind}/{conn}"]
                labels, table = v.Components(of, conn)
                assert len(table) == row["count"], (key, kind, conn)
                assert sha(labels) == row["labels_sha256"] and sha(table) == row["table_sha256"], (key, kind, conn)
                print(f"{key} {kind} {conn}: K {len(table)}, {v.components_ms():.3f} ms")
    finally:
        v.close()


# ---- frames, staleness, trim, refusals ---------------------------------------------------------------------------------------------------
def test_three_frames_in_flight_each_get_their_own_labels(dxv, bunny):
    vb, ib, _ = bunny
    v = dxv.Voxelizer(0)
    try:
        v.InitFromArrays(vb, ib)
        plan = [(0, 32, dxv.MODE_REFERENCE, cr.SOLID, 6), (1, 24, dxv.MODE_PARITY, cr.EMPTY, 26), (2, 16, dxv.MODE_SURFACE, cr.EMPTY, 6)]
        for frame, N, mode, of, conn in plan:                           # no synchronisation between any of these
            v.Voxelize(N, mode, sync=False, frameIndex=frame)
            assert v.Components(of, conn, sync=False) is True
        v.SyncAll()
        seen = set()
        for frame, N, mode, of, conn in plan:
            v.SetFrame(frame)
            v.Sync()
            assert v.components_ms() > 0.0, frame
            want, wtable = cr.label(v.Grid(), of, conn)
            assert np.array_equal(v.ComponentLabels(), want) and np.array_equal(v.ComponentTable(), wtable) and len(wtable) >= 1, frame
            assert v.components_info() == (len(wtable), of, conn)
            seen.add(v.component_device_ptrs()[0])
        assert len(seen) == 3
    finally:
        v.close()


def test_labels_are_stale_after_voxelize_fill_expand_and_select_and_trim_keeps_them(dxv):
    from dxrvoxelizer_amd import meshes
    vb, ib = meshes.cube()
    v = dxv.Voxelizer(0)
    lib, ctx = v._lib, v._ctx

    def stale():
        with pytest.raises(dxv.DxvError, match="stale"):
            v.components_info()
        assert lib.dxv_components_labels_device_ptr(ctx) is None and "stale" in lib.dxv_last_error(ctx).decode()
        assert lib.dxv_components_table_device_ptr(ctx) is None and "stale" in lib.dxv_last_error(ctx).decode()
        assert lib.dxv_components_labels_bytes(ctx) == 0 and lib.dxv_components_table_bytes(ctx) == 0
        buf = np.empty(16 ** 3, np.uint32)
        assert lib.dxv_components_labels_download(ctx, buf.ctypes.data_as(C.c_void_p), buf.nbytes) == 1 and "stale" in lib.dxv_last_error(ctx).decode()
        assert lib.dxv_components_table_download(ctx, buf.ctypes.data_as(C.c_void_p), 24) == 1 and "stale" in lib.dxv_last_error(ctx).decode()
        with pytest.raises(dxv.DxvError, match="stale"):                # ... and nothing can be selected from them
            v.SelectComponents(cr.LARGEST)

    try:
        v.InitFromArrays(vb, ib)
        v.Voxelize(16, dxv.MODE_SURFACE)
        first = v.Components(cr.EMPTY, 6)
        assert len(first[1]) == 1 and first[1][0]["voxels"] == 14 ** 3 and first[1][0]["flags"] == 0      # the cube's shell lies on the grid's border: its inside
        v.trim()                                                       # the scratch goes, labels and table stay
        assert np.array_equal(v.ComponentLabels(), first[0]) and np.array_equal(v.ComponentTable(), first[1])
        again = v.Components(cr.EMPTY, 6)                              # ... and the next build is identical
        assert np.array_equal(again[0], first[0]) and np.array_equal(again[1], first[1])
        v.Fill()
        stale()
        v.Components()
        v.Octree()
        v.OctreeExpand()
        stale()
        v.Components()
        v.SelectComponents(cr.BORDER)
        stale()
        v.Components()
        v.Voxelize(16)
        stale()
    finally:
        v.close()


def test_components_refuse_with_a_message_and_leave_the_grid_untouched(dxv):
    from dxrvoxelizer_amd import meshes
    vb, ib = meshes.tetrahedron()
    v = dxv.Voxelizer(0)
    lib, ctx = v._lib, v._ctx

    def last():
        return lib.dxv_last_error(ctx).decode()

    def build_refused(of, conn, text):
        for fn in (lib.dxv_components_async, lib.dxv_components):
            assert fn(ctx, of, conn) == 1 and text in last(), (text, last())

    def select_refused(rule, arg, text):
        for fn in (lib.dxv_components_select_async, lib.dxv_components_select):
            assert fn(ctx, rule, arg) == 1 and text in last(), (text, last())

    try:
        build_refused(0, 6, "no grid yet")
        select_refused(0, 0, "no components yet")
        assert lib.dxv_components_info(ctx, None, None, None) == 1 and "no components yet" in last()
        assert lib.dxv_components_labels_device_ptr(ctx) is None and lib.dxv_components_labels_bytes(ctx) == 0
        v.InitFromArrays(vb, ib)
        v.Voxelize(16, z0=4, nz=8)
        g = v.Grid()
        build_refused(0, 6, "slab")
        assert np.array_equal(v.Grid(), g)
        v.VoxelizeInterleaved(16, 0, 2, 4)
        g = v.Grid()
        build_refused(0, 6, "share")
        assert np.array_equal(v.Grid(), g)
        v.Voxelize(16)
        g = v.Grid()
        build_refused(2, 6, "unknown kind")
        build_refused(-1, 26, "unknown kind")
        build_refused(0, 18, "connectivity")
        build_refused(1, 0, "connectivity")
        select_refused(0, 0, "no components yet")                      # a select without labels
        labels, table = v.Components()
        select_refused(3, 0, "unknown rule")
        select_refused(-1, 0, "unknown rule")
        select_refused(cr.LARGEST, 5, "arg must be 0")
        select_refused(cr.BORDER, 1, "arg must be 0")
        assert np.array_equal(v.Grid(), g)                             # nothing was written
        assert np.array_equal(v.ComponentLabels(), labels)             # ... and the labels are still current
        buf = np.empty(16 ** 3 + 1, np.uint32)
        assert lib.dxv_components_labels_download(ctx, buf.ctypes.data_as(C.c_void_p), buf.nbytes) == 1 and f"expected {4 * 16 ** 3} bytes" in last()
        assert lib.dxv_components_table_download(ctx, None, 24 * len(table)) == 1
        assert lib.dxv_components_ms(ctx, None) == 1
        assert lib.dxv_components_select(ctx, cr.MIN_VOXELS, 0) == 0   # the same call with what it asks for: everything is kept
        assert np.array_equal(v.Grid(), g) and v.select_info() == (len(table), 0, 0)
    finally:
        v.close()
