"""The line-of-sight map on the GPU (include/dxv.h: dxv_sight*): the device's map (uint32 per voxel), its tally and the grid after dxv_sight_fill
equal, as bytes, what the rule gives for the grid -- by the host library (tests/sight_host.py: the product's routines run word by word, held to
the restatements by tests/test_sight_rule.py) and, where noted, by restatement (b) of tests/sight_restated.py -- on the smallest shapes that
still reach each mechanism: a grid of members only; one non-member at the places where a carry crosses a word or enters at a row's open end; a
plate with a pinhole; a closed hollow box and the same box with a hole; a T-slot and its pull axes; every single direction and every axis pair;
the widest row group forced at two sides; five words in a group of eight; the call's discipline; the refusals; the bunny at 64^3."""
import ctypes as C

import numpy as np
import pytest

import grid_sides as gs
import sight_host as sh
import sight_restated as sr
from raycast_restated import write_grid

pytestmark = pytest.mark.gpu
SOLID, EMPTY, ALL = sr.SOLID, sr.EMPTY, sr.ALL
PAIRS = [sr.axis_bits(a) for a in range(13)]


@pytest.fixture(scope="module")
def dxv(dxvlib):
    import dxrvoxelizer_amd
    return dxrvoxelizer_amd


@pytest.fixture(scope="module")
def writer(dxv, bunny):
    """the one Voxelizer, on the bunny, whose frame the grids of this file are written into"""
    vb, ib, _ = bunny
    v = dxv.Voxelizer(0)
    v.InitFromArrays(vb, ib)
    yield v
    v.close()


def load(v, g):
    if v.stats()["grid_dim"] != g.shape[0]:
        v.Voxelize(g.shape[0])
    write_grid(v, g)


def check(v, g, of, directions=ALL, restated=False, what="", want=None):
    """Sight of the selected frame, which holds g: map and tally against the host library (want: its answer, where the caller has it) and,
    with `restated`, form (b); returns (map, tally)"""
    want_map, want_tally = want if want is not None else sh.sight(g, of, directions)
    key = (what, g.shape[0], of, hex(directions))
    field = v.Sight(of, directions)
    assert field.dtype == np.uint32 and field.shape == g.shape and field.tobytes() == want_map.tobytes(), (key, int(np.count_nonzero(field != want_map)))
    tally = v.SightTally()
    assert sr.same_tally(tally, want_tally), (key, tally, want_tally)
    if restated:
        assert field.tobytes() == sr.sight(g, of, directions).tobytes() and sr.same_tally(tally, sr.tally(g, of, field, directions)), key
    info = v.SightInfo()
    assert info["of"] == of and info["directions"] == directions, key
    return field, tally


# ---- members only ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [2, 64, 66])
def test_a_grid_of_members_only(writer, N):
    v = writer
    for g, of in ((np.zeros((N, N, N), np.uint8), EMPTY), (np.full((N, N, N), 0xFF, np.uint8), SOLID)):
        load(v, g)
        field, tally = check(v, g, of, restated=True, what="members only")
        assert (field == ALL).all() and tally["members"] == N ** 3 == tally["count"][26] and not tally["neither"].any()
        field, tally = check(v, g, 1 - of, restated=True, what="no member")
        assert not field.any() and tally["members"] == 0 and not tally["seen"].any() and not tally["count"].any()


# ---- one non-member: its 26 shadow lines ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("x", [0, 1, 63, 64, 65])
def test_one_non_member_casts_26_shadow_lines(writer, x):
    """the carry across the word boundary both ways, and the carry that enters at bit N % 64 of a row's open end for dx = -1"""
    N = 66
    v = writer
    for z, y in ((z, y) for z in (0, 33, 65) for y in (0, 33, 65)):
        g = np.zeros((N, N, N), np.uint8)
        g[z, y, x] = 0x40
        load(v, g)
        field, tally = check(v, g, EMPTY, what=("one non-member", z, y, x))
        want = np.full((N, N, N), ALL, np.uint32)
        want[z, y, x] = 0
        for b in sr.BITS:                                               # behind the non-member along d, up to the border: not seen along d
            dx, dy, dz = sr.direction(b)
            k = 1
            while 0 <= z + k * dz < N and 0 <= y + k * dy < N and 0 <= x + k * dx < N:
                want[z + k * dz, y + k * dy, x + k * dx] &= np.uint32(~(1 << b) & 0xFFFFFFFF)
                k += 1
        assert field.tobytes() == want.tobytes(), (z, y, x)
        assert tally["members"] == N ** 3 - 1 and tally["count"][0] == 0


# ---- the plate, the boxes, the slot ---------------------------------------------------------------------------------------------------------
def test_a_plate_with_a_pinhole(writer):
    N, hole = 16, (5, 9)
    g = sr.plate_with_pinhole(N, hole)
    v = writer
    load(v, g)
    field, tally = check(v, g, EMPTY, restated=True, what="plate")
    down, up = 1 << sr.bit(0, 0, -1), 1 << sr.bit(0, 0, 1)             # rays travelling down z come from above
    below = (field[:N // 2] & down) != 0
    assert below[:, hole[0], hole[1]].all() and below.sum() == N // 2 and ((field[N // 2 + 1:] & down) != 0).all()
    assert ((field[N // 2 + 1:] & up) != 0).sum() == N // 2 - 1 and ((field[:N // 2] & up) != 0).all()
    assert tally["neither"][8] == 0                                     # everything is seen from above or from below
    one, _ = check(v, g, EMPTY, down, restated=True, what="plate from above")
    assert one.tobytes() == (field & np.uint32(down)).tobytes()


def test_a_closed_hollow_box_and_the_same_box_with_a_hole(writer):
    N, lo, hi = 16, 2, 6
    g = gs.hollow_box(N, lo, hi)
    want = sr.tally(g, EMPTY, sr.sight(g, EMPTY), ALL)
    assert want["count"][0] == (hi - lo - 1) ** 3 > 0 and want["count"][26] > 0        # (the conditions, from the restatement)
    v = writer
    load(v, g)
    field, tally = check(v, g, EMPTY, restated=True, what="hollow box")
    inside = (slice(lo + 1, hi), slice(lo + 1, hi), slice(lo + 1, hi))
    assert not field[inside].any() and tally["count"][0] == (hi - lo - 1) ** 3 and tally["count"][26] > 0
    shell, stally = check(v, g, SOLID, restated=True, what="hollow box, the shell")
    assert stally["members"] == int(g.sum()) and not shell[inside].any()
    g[hi, 4, 4] = 0                                                     # a face voxel of the top removed: exactly the lines through that hole
    load(v, g)
    field, tally = check(v, g, EMPTY, restated=True, what="box with a hole")
    lit = np.zeros((N, N, N), bool)
    for b in sr.BITS:
        dx, dy, dz = sr.direction(b)
        if dz >= 0:
            continue                                                    # only rays travelling down z enter through a hole in the top
        k = 1
        while lo < hi + k * dz < hi and lo < 4 + k * dy < hi and lo < 4 + k * dx < hi:
            lit[hi + k * dz, 4 + k * dy, 4 + k * dx] = True
            assert field[hi + k * dz, 4 + k * dy, 4 + k * dx] == 1 << b
            k += 1
    assert lit[inside].sum() > 3 and ((field[inside] != 0) == lit[inside]).all()
    assert tally["count"][0] == (hi - lo - 1) ** 3 - lit[inside].sum()


def test_a_t_slot_and_its_pull_axes(dxv, writer):
    g = sr.t_slot(16)
    v = writer
    load(v, g)
    field, tally = check(v, g, EMPTY, restated=True, what="t slot")
    assert tally["neither"][0] == 0 and tally["neither"][2] > 0 and tally["neither"][8] > 0
    axes = dxv.sight_axes(tally)
    assert [a["axis"] for a in axes][0] == 0 and axes[0]["direction"] == (1, 0, 0) and axes[0]["neither"] == 0 and axes[1]["neither"] > 0
    assert sorted(a["axis"] for a in axes) == list(range(13)) and all(a["bits"] == sr.axis_bits(a["axis"]) for a in axes)
    assert dxv.sight_bit(1, 0, 0) == 14 and dxv.sight_bit(0, 0, -1) == 4 and dxv.SIGHT_ALL == ALL
    worst = axes[-1]
    assert worst["direction"] == (0, 1, 0) and worst["neither"] == tally["members"]
    v.SightFill(worst["bits"])
    filled = v.Grid()
    assert filled.tobytes() == sr.sight_fill(g, EMPTY, field, worst["bits"]).tobytes() == sh.sight_fill(g, EMPTY, worst["bits"], field).tobytes()
    assert filled.all()                                                 # the slot is gone
    # the pull along z: only the wings beside the neck are filled, and nothing is hidden afterwards
    load(v, g)
    field, tally = check(v, g, EMPTY, what="t slot again")
    v.SightFill(sr.axis_bits(8))
    filled = v.Grid()
    assert filled.tobytes() == sr.sight_fill(g, EMPTY, field, sr.axis_bits(8)).tobytes()
    assert int(filled.sum()) - int(g.sum()) == tally["neither"][8] == 16 * 4 * 6
    _, after = check(v, filled, EMPTY, sr.axis_bits(8), restated=True, what="t slot filled")
    assert after["count"][0] == 0 and after["neither"][8] == 0


# ---- every direction, every pair ------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def random66():
    g = gs.random_grid(66, 0.3)
    out = {}
    for of in (SOLID, EMPTY):
        field, tally = sh.sight(g, of, ALL)
        restated = sr.sight(g, of, ALL)
        want = sr.tally(g, of, restated, ALL)
        assert field.tobytes() == restated.tobytes() and sr.same_tally(tally, want)
        assert np.count_nonzero(want["count"]) >= 10 and len({int(want["seen"][b]) for b in sr.BITS}) >= 2      # (the conditions, from the restatement)
        out[of] = (field, tally)
    return g, out


@pytest.mark.parametrize("of", [SOLID, EMPTY])
def test_every_single_direction_and_every_pair(writer, random66, of):
    g, full = random66
    v = writer
    load(v, g)
    field, tally = check(v, g, of, want=full[of], what="random 0.3")
    for directions in [1 << b for b in sr.BITS] + PAIRS:
        part = v.Sight(of, directions)
        assert part.tobytes() == (field & np.uint32(directions)).tobytes(), hex(directions)
        t = v.SightTally()
        assert sr.same_tally(t, sr.tally(g, of, part, directions)), hex(directions)
        asked = np.array([directions >> b & 1 for b in range(27)], bool)
        assert not t["seen"][~asked].any() and (t["seen"][asked] == tally["seen"][asked]).all()
        both = np.array([directions & p == p for p in PAIRS], bool)
        assert not t["neither"][~both].any() and (t["neither"][both] == tally["neither"][both]).all()
        assert not t["count"][bin(directions).count("1") + 1:].any() and t["count"].sum() == t["members"] == tally["members"]


# ---- the row groups -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [66, 130])
def test_the_widest_row_group_forced(dxv, writer, N):
    """a group of 16 lanes needs a side above 512 in production: option sightgroup forces it here, and every width in between"""
    g = gs.random_grid(N, 0.3)
    v = writer
    load(v, g)
    want = sh.sight(g, EMPTY, ALL)
    try:
        plain, _ = check(v, g, EMPTY, want=want, what="group 0")
        for group in (16, 8, 4, 2, 1):
            v.set_option("sightgroup", group)
            forced, _ = check(v, g, EMPTY, want=want, what=f"group {group}")
            assert forced.tobytes() == plain.tobytes()
        for bad in (3, 32, -1):
            with pytest.raises(dxv.DxvError, match="sightgroup"):
                v.set_option("sightgroup", bad)
    finally:
        v.set_option("sightgroup", 0)


def test_five_words_in_a_group_of_eight(writer):
    g = gs.random_grid(258, 0.3)
    v = writer
    load(v, g)
    want = sr.tally(g, EMPTY, sr.sight(g, EMPTY), ALL)
    assert np.count_nonzero(want["count"]) >= 10 and len({int(want["seen"][b]) for b in sr.BITS}) >= 2      # (the conditions, from the restatement)
    check(v, g, EMPTY, restated=True, what="258")


# ---- discipline -----------------------------------------------------------------------------------------------------------------------------
def test_two_frames_enqueued_back_to_back(dxv, bunny):
    vb, ib, _ = bunny
    v = dxv.Voxelizer(0)
    try:
        v.InitFromArrays(vb, ib)
        plan = [(0, 24, dxv.MODE_REFERENCE, SOLID, ALL), (1, 18, dxv.MODE_SURFACE, EMPTY, PAIRS[8]), (2, 16, dxv.MODE_REFERENCE, EMPTY, ALL)]
        for frame, N, mode, of, directions in plan:                     # no synchronisation between any of these
            v.Voxelize(N, mode, sync=False, frameIndex=frame)
            assert v.Sight(of, directions, sync=False) is True
        v.SyncAll()
        seen = set()
        for frame, N, mode, of, directions in plan:
            v.SetFrame(frame)
            v.Sync()
            g = v.Grid()
            want_map, want_tally = sh.sight(g, of, directions)
            assert g.any() and v.SightField().tobytes() == want_map.tobytes() and sr.same_tally(v.SightTally(), want_tally), frame
            info = v.SightInfo()
            assert info["ms"] > 0.0 and info["of"] == of and info["directions"] == directions, frame
            seen.add(v.sight_device_ptr())
        assert len(seen) == 3
    finally:
        v.close()


def test_a_small_grid_after_a_larger_one(writer):
    """the scratch and the map are reused from the larger grid"""
    v = writer
    for N in (72, 6):
        g = gs.random_grid(N, 0.3)
        load(v, g)
        for of in (SOLID, EMPTY):
            check(v, g, of, restated=True, what="after a larger grid")


def test_the_map_is_stale_once_the_grid_is_rewritten(dxv):
    from dxrvoxelizer_amd import meshes
    vb, ib = meshes.cube()
    v = dxv.Voxelizer(0)
    lib, ctx = v._lib, v._ctx

    def stale():
        for read in (v.SightField, v.SightTally, v.SightInfo, v.sight_device_ptr, lambda: v.SightFill(ALL)):
            with pytest.raises(dxv.DxvError, match="stale"):
                read()
        assert lib.dxv_sight_device_ptr(ctx) is None and "stale" in lib.dxv_last_error(ctx).decode() and lib.dxv_sight_bytes(ctx) == 0
        buf = np.empty(16 ** 3, np.uint32)
        assert lib.dxv_sight_download(ctx, buf.ctypes.data_as(C.c_void_p), buf.nbytes) == 1 and "stale" in lib.dxv_last_error(ctx).decode()

    try:
        v.InitFromArrays(vb, ib)
        v.Voxelize(16, dxv.MODE_SURFACE)
        for edit in (lambda: v.Voxelize(16, dxv.MODE_SURFACE), lambda: v.Fill(), lambda: v.Morph(dxv.MORPH_ERODE, 1), lambda: v.SightFill(PAIRS[0])):
            field = v.Sight(SOLID, ALL)
            assert field.any() and lib.dxv_sight_bytes(ctx) == 4 * 16 ** 3
            v.Components(EMPTY, 6)                                     # what only reads the grid leaves the map current
            v.Thickness(SOLID, 9)
            v.Access(EMPTY, 6, 65)
            assert v.SightField().tobytes() == field.tobytes()
            edit()
            stale()
            for other in (v.ThicknessField, v.AccessField):
                with pytest.raises(dxv.DxvError, match="stale"):       # the other products are stale with it
                    other()
            v.Voxelize(16, dxv.MODE_SURFACE)
    finally:
        v.close()


def test_sight_refuses_with_a_message_and_leaves_everything_untouched(dxv):
    from dxrvoxelizer_amd import meshes
    vb, ib = meshes.tetrahedron()
    v = dxv.Voxelizer(0)
    lib, ctx = v._lib, v._ctx

    def refused(args, text):
        for fn in (lib.dxv_sight_async, lib.dxv_sight):
            assert fn(ctx, *args) == 1 and text in lib.dxv_last_error(ctx).decode(), (text, lib.dxv_last_error(ctx).decode())

    def fill_refused(directions, text):
        for fn in (lib.dxv_sight_fill_async, lib.dxv_sight_fill):
            assert fn(ctx, directions) == 1 and text in lib.dxv_last_error(ctx).decode(), (text, lib.dxv_last_error(ctx).decode())

    try:
        refused((0, ALL), "no grid yet")                                # no launch
        assert lib.dxv_sight_device_ptr(ctx) is None and "no line-of-sight map yet" in lib.dxv_last_error(ctx).decode()
        assert lib.dxv_sight_bytes(ctx) == 0
        assert lib.dxv_sight_info(ctx, None, None, None) == 1 and "no line-of-sight map yet" in lib.dxv_last_error(ctx).decode()
        fill_refused(ALL, "no line-of-sight map yet")
        v.InitFromArrays(vb, ib)
        v.Voxelize(16)
        g = v.Grid()
        with pytest.raises(dxv.DxvError, match="no line-of-sight map yet"):
            v.SightField()
        words = np.empty(68, np.uint64)
        assert lib.dxv_sight_tally_download(ctx, words.ctypes.data_as(C.c_void_p), words.nbytes) == 1 and "no line-of-sight map yet" in lib.dxv_last_error(ctx).decode()
        for of in (-1, 2):
            refused((of, ALL), "unknown kind")
        for directions in (0, 1 << 13, ALL | 1 << 13, 1 << 27, 0x80000000, 0xFFFFFFFF):
            refused((0, directions), "not a non-empty subset of DXV_SIGHT_ALL")
        made = PAIRS[8] | PAIRS[0]
        field = v.Sight(SOLID, made)
        tally = v.SightTally()
        refused((2, ALL), "unknown kind")                               # a refusal leaves the map of before current
        refused((0, 0), "not a non-empty subset")
        for directions in (0, ALL, PAIRS[2], made | 1 << 13, 1 << 27):
            fill_refused(directions, "not a non-empty subset of the")   # not a subset of the map's directions
        want_map, want_tally = sh.sight(g, SOLID, made)
        assert v.SightField().tobytes() == field.tobytes() == want_map.tobytes() and sr.same_tally(v.SightTally(), tally) and sr.same_tally(tally, want_tally)
        buf = np.empty(16 ** 3 + 1, np.uint32)                          # wrong download sizes
        assert lib.dxv_sight_download(ctx, buf.ctypes.data_as(C.c_void_p), buf.nbytes) == 1 and "expected" in lib.dxv_last_error(ctx).decode()
        assert lib.dxv_sight_download(ctx, None, 4 * 16 ** 3) == 1
        assert lib.dxv_sight_tally_download(ctx, words.ctypes.data_as(C.c_void_p), words.nbytes - 8) == 1 and "expected 544 bytes" in lib.dxv_last_error(ctx).decode()
        assert lib.dxv_sight_tally_download(ctx, None, 544) == 1
        assert lib.dxv_sight_info(ctx, None, None, None) == 0
        assert np.array_equal(v.Grid(), g) and v.SightField().tobytes() == field.tobytes()
        v.Voxelize(16, z0=4, nz=8)                                      # a slab
        refused((0, ALL), "slab")
        fill_refused(made, "stale")
        v.Voxelize(1026)
        refused((0, 1), "at most 1024^3")
        assert lib.dxv_sight_bytes(ctx) == 0
    finally:
        v.close()


def test_after_trim_the_map_stays_and_the_call_works_again(dxv, bunny):
    vb, ib, _ = bunny
    v = dxv.Voxelizer(0)
    try:
        v.InitFromArrays(vb, ib)
        v.Voxelize(34)
        g = v.Grid()
        field, tally = check(v, g, EMPTY, what="before trim")
        v.trim()
        assert v.SightField().tobytes() == field.tobytes() and sr.same_tally(v.SightTally(), tally)
        v.SightFill(PAIRS[8])                                           # the edit reads the map alone: the trim has left it
        assert v.Grid().tobytes() == sr.sight_fill(g, EMPTY, field, PAIRS[8]).tobytes()
        check(v, v.Grid(), SOLID, PAIRS[3], what="after trim")
    finally:
        v.close()


# ---- the bunny ------------------------------------------------------------------------------------------------------------------------------
def test_the_bunny_at_64(dxv, writer):
    v = writer
    v.Voxelize(64, dxv.MODE_SURFACE)
    v.Fill()
    g = v.Grid()
    assert g.any() and not g.all()
    field, tally = check(v, g, EMPTY, what="bunny")
    assert tally["members"] == int((g == 0).sum()) and 0 < tally["neither"].min() < tally["neither"].max()     # (no axis demoulds a bunny)
    again = v.Sight(EMPTY, ALL)
    assert again.tobytes() == field.tobytes()
