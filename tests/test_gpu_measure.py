"""The integral measures of a labelling on the GPU (include/dxv.h: dxv_measure*): the device's table equals the numpy restatement
(tests/measure_restated.py) AS BYTES, for both kinds and both connectivities -- for grids written through the frame's grid pointer at the sides
where the pack and the rows change path, for every lane its own label and for one label in every wave, for sums that leave 32 bits, for
meshes, for large grids against committed hashes (tests/golden/measure.json, tests/gen_measure_fixtures.py); the Euler number and the pieces
the device counts do not change under the device's own thinning; Betti; three frames in flight; the mask rebuilt after a trim; staleness;
and the calls refuse what they must."""
import ctypes as C
import itertools
import json
import os

import numpy as np
import pytest

import components_restated as cr
import fill_restated as fr
import grid_sides as gs
import measure_restated as ms
import thin_shapes as ts
from conftest import GOLD, load_mesh
from raycast_restated import write_grid
from test_gpu_components import sha

pytestmark = pytest.mark.gpu

CASES = list(itertools.product((cr.SOLID, cr.EMPTY), (6, 26)))


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


def plain(record):
    """a record as a tuple of Python integers and lists"""
    return tuple(np.asarray(record[n]).tolist() for n in ms.RECORD.names)


def check(v, g, what, cases=CASES):
    """the measures of the selected frame's grid, which holds g, against the restatement of g: {(of, conn): table}"""
    out = {}
    for of, conn in cases:
        labelling = ms.label(g, of, conn)
        want = ms.measure(g, of, conn, labelling)
        assert v.Components(of, conn, sync=False) is True
        got = v.Measure()
        assert v.components_info() == (len(want) - 1, of, conn), (what, of, conn)
        assert got.dtype == ms.RECORD and got.shape == want.shape, (what, of, conn)
        assert got.tobytes() == want.tobytes(), (what, of, conn, [n for n in ms.RECORD.names if not np.array_equal(got[n], want[n])])
        assert v._lib.dxv_measure_table_bytes(v._ctx) == 96 * len(want) and v.measure_device_ptr(), (what, of, conn)
        if of == cr.SOLID:
            assert int(got[0]["voxels"]) == v.CountSolid(), (what, conn)
        out[of, conn] = got
    return out


# ---- written grids -------------------------------------------------------------------------------------------------------------------------
# 2: all border; 64: one full word; 66: a word and two bits, the guarded pack path; 96: a word and a half
@pytest.mark.parametrize("N", [2, 64, 66, 96])
def test_written_grids_equal_restatement(writer, N):
    v = writer
    v.Voxelize(N)
    seen = 0
    for name, g in gs.grids(N):
        seen += 1
        write_grid(v, g)
        got = check(v, g, (N, name))
        if name == "random 0.3" and N > 2:
            assert len(got[cr.SOLID, 6]) > 100                          # many labels in one wave
    assert seen == (5 if N >= 6 else 4)
    assert np.array_equal(v.Grid(), g)                                  # measuring edits nothing
    assert v.measure_ms() > 0.0


def test_checkerboard_one_voxel_and_the_empty_grid(writer):
    v = writer
    N = 32
    v.Voxelize(N)
    g = cr.checkerboard(N)
    write_grid(v, g)
    got = check(v, g, "checkerboard")
    assert len(got[cr.SOLID, 6]) == N ** 3 // 2 + 1 and len(got[cr.SOLID, 26]) == 2      # every lane its own label; one component
    assert (got[cr.SOLID, 6]["euler"][1:] == 1).all() and (got[cr.SOLID, 6]["faces"][1:] == 6).all()
    g = cr.one_voxel(N)
    write_grid(v, g)
    got = check(v, g, "one voxel")
    assert plain(got[cr.SOLID, 26][1]) == (1, [N // 2, 0, N - 1], [(N // 2) ** 2, 0, (N - 1) ** 2], [0, 0, (N - 1) * (N // 2)], 6, 1)
    g = np.zeros((N, N, N), np.uint8)
    write_grid(v, g)
    got = check(v, g, "empty")
    assert got[cr.SOLID, 6].tobytes() == bytes(96) and got[cr.SOLID, 26].tobytes() == bytes(96)      # K = 0: one all-zero record


def test_the_eight_flips_of_a_random_grid(writer):
    v = writer
    N = 34
    v.Voxelize(N)
    g = fr.random_walls(N, 0.3, 34, bytes_other_than_one=True)
    first = None
    for fx, fy, fz in itertools.product((False, True), repeat=3):
        f = np.ascontiguousarray(g[::-1 if fz else 1, ::-1 if fy else 1, ::-1 if fx else 1])
        write_grid(v, f)
        got = check(v, f, ("flip", fx, fy, fz))
        chi = {k: int(t[0]["euler"]) for k, t in got.items()}
        first = first or chi
        assert chi == first                                             # the ownership of cells is not symmetric; the sums are


def test_sums_beyond_32_bits_on_an_all_solid_grid(writer):
    v = writer
    N = 130
    v.Voxelize(N)
    g = np.full((N, N, N), 0xFF, np.uint8)
    write_grid(v, g)
    got = check(v, g, "all 0xFF 130", [(cr.SOLID, 6), (cr.SOLID, 26)])
    s1, s2 = N * (N - 1) // 2, (N - 1) * N * (2 * N - 1) // 6
    assert s2 * N * N > 2 ** 32
    for t in got.values():
        assert plain(t[1]) == (N ** 3, [s1 * N * N] * 3, [s2 * N * N] * 3, [s1 * s1 * N] * 3, 6 * N * N, 1)
        assert t[0] == t[1]


# ---- meshes --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["bunny", "dragon", "turingbowl"])
def test_mesh_grids_equal_restatement(dxv, name):
    vb, ib, _ = load_mesh(name)
    v = dxv.Voxelizer(0)
    try:
        v.InitFromArrays(vb, ib)
        for N, mode, fill, cases in ((64, dxv.MODE_REFERENCE, False, CASES), (64, dxv.MODE_SURFACE, True, [(cr.SOLID, 26), (cr.EMPTY, 6)]),
                                     (128, dxv.MODE_REFERENCE, False, [(cr.SOLID, 26), (cr.EMPTY, 6)])):
            v.Voxelize(N, mode)
            if fill:
                v.Fill()
            g = v.Grid()
            assert g.any()
            got = check(v, g, (name, N, mode, fill), cases)
            t = got[cr.SOLID, 26]
            print(f"{name} {N} mode {mode} fill {fill}: K {len(t) - 1}, voxels {int(t[0]['voxels'])}, faces {int(t[0]['faces'])}, euler {int(t[0]['euler'])}, {v.measure_ms():.3f} ms")
    finally:
        v.close()


@pytest.mark.parametrize("key", ["bunny/256", "torus1m/512"])
def test_large_grids_equal_committed_hashes(dxv, key):
    from dxrvoxelizer_amd import meshes
    with open(os.path.join(GOLD, "measure.json")) as fh:
        want = json.load(fh)[key]
    name, N = key.split("/")
    vb, ib = meshes.torus() if name == "torus1m" else load_mesh(name)[:2]
    v = dxv.Voxelizer(0)
    try:
        v.InitFromArrays(vb, ib)
        v.Voxelize(int(N), dxv.MODE_REFERENCE)
        assert sha(v.Grid()) == want["grid_sha256"], f"{key}: the grid is not the one the fixture was made from"
        for of, conn, tag in ((cr.SOLID, 26, "solid/26"), (cr.EMPTY, 6, "empty/6")):
            row = want[tag]
            assert v.Components(of, conn, sync=False) is True
            table = v.Measure()
            assert len(table) == row["count"] + 1, (key, tag)
            assert {n: np.asarray(table[0][n]).tolist() for n in ms.RECORD.names} == row["record0"], (key, tag)
            assert sha(table) == row["table_sha256"], (key, tag)
            print(f"{key} {tag}: K {len(table) - 1}, measure {v.measure_ms():.3f} ms, components {v.components_ms():.3f} ms")
    finally:
        v.close()


# ---- the device's own thinning as second oracle ---------------------------------------------------------------------------------------------
def test_thinning_on_the_device_keeps_the_euler_number_and_the_pieces(dxv, writer):
    v = writer

    def chi_and_pieces():
        assert v.Components(cr.SOLID, 26, sync=False) is True
        t = v.Measure()
        return int(t[0]["euler"]), len(t) - 1, int(t[0]["voxels"])

    v.Voxelize(48)
    write_grid(v, fr.random_walls(48, 0.3, 48, bytes_other_than_one=True))
    before = chi_and_pieces()
    v.Thin(dxv.THIN_KERNEL)
    after = chi_and_pieces()
    assert after[:2] == before[:2] and after[2] < before[2] and before[0] < 0 and before[1] > 1
    v.Voxelize(64, dxv.MODE_SURFACE)
    v.Fill()
    before = chi_and_pieces()
    v.Thin(dxv.THIN_KERNEL)
    after = chi_and_pieces()
    assert after[:2] == before[:2] and after[2] < before[2]


def test_betti_of_a_torus_and_a_hollow_box(dxv, writer):
    v = writer
    v.Voxelize(32)
    write_grid(v, ts.torus(32))
    assert v.Betti() == (1, 1, 0)
    assert v.components_info() == (1, cr.SOLID, 26) and int(v.MeasureTable()[0]["euler"]) == 0      # the solid labelling and its measure stay current
    write_grid(v, gs.hollow_box(32, 1, 30))
    assert v.Betti() == (1, 0, 1)
    write_grid(v, ts.ball(32))
    assert v.Betti() == (1, 0, 0)


# ---- frames, trim, staleness, refusals -----------------------------------------------------------------------------------------------------
def test_three_frames_in_flight_each_get_their_own_table(dxv, bunny):
    vb, ib, _ = bunny
    v = dxv.Voxelizer(0)
    try:
        v.InitFromArrays(vb, ib)
        plan = [(0, 32, dxv.MODE_REFERENCE, cr.SOLID, 6), (1, 24, dxv.MODE_PARITY, cr.EMPTY, 26), (2, 16, dxv.MODE_SURFACE, cr.SOLID, 26)]
        for frame, N, mode, of, conn in plan:                           # no synchronisation between any of these but the labelling's read of K
            v.Voxelize(N, mode, sync=False, frameIndex=frame)
            assert v.Components(of, conn, sync=False) is True
            assert v.Measure(sync=False) is True
        v.SyncAll()
        seen = set()
        for frame, N, mode, of, conn in plan:
            v.SetFrame(frame)
            v.Sync()
            assert v.measure_ms() > 0.0, frame
            want = ms.measure(v.Grid(), of, conn)
            assert v.MeasureTable().tobytes() == want.tobytes() and len(want) >= 2, frame
            seen.add(v.measure_device_ptr())
        assert len(seen) == 3
    finally:
        v.close()


@pytest.mark.parametrize("N,of,conn", [(64, cr.SOLID, 26), (66, cr.EMPTY, 6)])
def test_measure_after_trim_packs_the_mask_again(dxv, bunny, N, of, conn):
    vb, ib, _ = bunny
    v = dxv.Voxelizer(0)
    try:
        v.InitFromArrays(vb, ib)
        v.Voxelize(N)
        g = v.Grid()
        want = ms.measure(g, of, conn)
        assert v.Components(of, conn, sync=False) is True
        first = v.Measure()
        assert first.tobytes() == want.tobytes()
        v.trim()
        assert v.MeasureTable().tobytes() == want.tobytes()            # the table stays, as the labels do
        assert v.Measure().tobytes() == want.tobytes()                 # ... and a measure without the labelling's mask makes it again
        assert v.Measure().tobytes() == want.tobytes()
        assert np.array_equal(v.Grid(), g)
    finally:
        v.close()


def test_the_measure_is_stale_exactly_when_its_labelling_is_and_after_a_new_one(dxv):
    from dxrvoxelizer_amd import meshes
    vb, ib = meshes.cube()
    v = dxv.Voxelizer(0)
    lib, ctx = v._lib, v._ctx

    def measured():
        v.Components(cr.SOLID, 26, sync=False)
        assert len(v.Measure()) >= 2 and lib.dxv_measure_table_bytes(ctx) >= 192

    def stale():
        with pytest.raises(dxv.DxvError, match="stale"):
            v.MeasureTable()
        assert lib.dxv_measure_table_device_ptr(ctx) is None and "stale" in lib.dxv_last_error(ctx).decode()
        assert lib.dxv_measure_table_bytes(ctx) == 0 and "stale" in lib.dxv_last_error(ctx).decode()
        buf = np.empty(2, ms.RECORD)
        assert lib.dxv_measure_table_download(ctx, buf.ctypes.data_as(C.c_void_p), buf.nbytes) == 1 and "stale" in lib.dxv_last_error(ctx).decode()

    try:
        v.InitFromArrays(vb, ib)
        v.Voxelize(16, dxv.MODE_SURFACE)
        for edit in (lambda: v.Voxelize(16, dxv.MODE_SURFACE), lambda: v.Fill(), lambda: v.Morph(dxv.MORPH_ERODE, 1), lambda: v.Thin(dxv.THIN_CURVE),
                     lambda: (v.Octree(), v.OctreeExpand()), lambda: v.SelectComponents(cr.LARGEST), lambda: v.Components(cr.SOLID, 26), lambda: v.Components(cr.EMPTY, 6)):
            measured()
            edit()
            stale()
            v.Voxelize(16, dxv.MODE_SURFACE)
    finally:
        v.close()


def test_measure_refuses_with_a_message_and_leaves_everything_untouched(dxv):
    from dxrvoxelizer_amd import meshes
    vb, ib = meshes.tetrahedron()
    v = dxv.Voxelizer(0)
    lib, ctx = v._lib, v._ctx

    def refused(text):
        for fn in (lib.dxv_measure_async, lib.dxv_measure):
            assert fn(ctx) == 1 and text in lib.dxv_last_error(ctx).decode(), (text, lib.dxv_last_error(ctx).decode())

    try:
        refused("no grid yet")                                          # no launch
        assert lib.dxv_measure_table_device_ptr(ctx) is None and "no measure yet" in lib.dxv_last_error(ctx).decode()
        assert lib.dxv_measure_table_bytes(ctx) == 0
        v.InitFromArrays(vb, ib)
        v.Voxelize(16)
        g = v.Grid()
        refused("no components yet")                                    # no labelling
        assert np.array_equal(v.Grid(), g)
        labels, table = v.Components(cr.SOLID, 6)
        with pytest.raises(dxv.DxvError, match="no measure yet"):
            v.MeasureTable()
        want = v.Measure()
        buf = np.empty(len(want) + 1, ms.RECORD)                        # a wrong download size
        assert lib.dxv_measure_table_download(ctx, buf.ctypes.data_as(C.c_void_p), buf.nbytes) == 1 and "expected" in lib.dxv_last_error(ctx).decode()
        assert lib.dxv_measure_table_download(ctx, None, want.nbytes) == 1
        assert np.array_equal(v.Grid(), g) and np.array_equal(v.ComponentLabels(), labels) and np.array_equal(v.ComponentTable(), table)
        assert v.MeasureTable().tobytes() == want.tobytes() == ms.measure(g, cr.SOLID, 6).tobytes()
        assert lib.dxv_measure_ms(ctx, None) == 1 and "ms is NULL" in lib.dxv_last_error(ctx).decode()
        v.Morph(dxv.MORPH_DILATE, 1)                                    # a stale labelling
        g = v.Grid()
        refused("stale")
        assert np.array_equal(v.Grid(), g)
        v.Voxelize(16, z0=4, nz=8)                                      # a slab
        refused("slab")
    finally:
        v.close()
