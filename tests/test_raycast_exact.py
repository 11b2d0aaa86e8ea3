"""The display pass (dxrvoxelizer_amd/csrc/raycast.hip, dxv_raycast.h: k_raycast, k_brick_summary, k_brick_empty) held byte for
byte on adversarial grids and cameras -- np.array_equal everywhere, no tolerance.

The product that is run (tests/raycast_restated.py):
  sizes    N in 2, 8, 10, 16, 50, 64, 72, 100, 128 -- the 64-bit row load and the byte loop, M = ceil(N / 8) of 1, 1, 2, 2, 7, 8, 9,
           13, 16 (runs of eight bricks that are partial, exactly full, full plus one), the smallest grid
  grids    per N, written through the frame's grid pointer: all zero, all 0xFF, random at densities 0.5 / 1e-2 / 1e-4 with bytes
           1..255, a checkerboard, a one-voxel slab on each of the six faces ("dense", 12 grids); one voxel at each of the 27
           combinations of {8k-1, 8k, 8k+1} per axis around one interior brick boundary (k = 8 where M > 8, the first brick of the
           second run, else M // 2; N = 2 and 8 have no interior boundary) and one at each of the eight corners ("single", up to
           35 grids); and the bunny voxelized at N
  cameras  dense grids and the bunny, nine views: default 160 x 90 and 1 x 1, oblique (-6, 3, 13) 17 x 33, inside 161 x 91, inside
           near a corner 17 x 33, one axis camera at 161 x 91 and 1 x 1 and the opposite-handed one at 17 x 33, far 17 x 33;
           single-voxel grids, three views: default 17 x 33, inside 17 x 33, one axis camera 161 x 91.  The six axis cameras (an
           eye on a coordinate axis looking at the centre) are dealt round the grids of a size.  "inside" sits inside solid in
           the all-0xFF grid.  1280 x 720 runs once, bunny at 256^3: tests/test_render_target.py.
  asserted (a) flags and summaries (dxv_debug_download) == the numpy restatement, every grid; (b) image with skipempty = 1 ==
           image with skipempty = 0, every grid and view; (c) RenderAsync into a device target == Render, the first view of every
           dense grid and the bunny; (d) the device's image == the oracle's march (oracle/orc.py render), every grid and view.
The CPU half runs the same grids and views at small windows (160 x 90 -> 32 x 18, 161 x 91 -> 33 x 19) through the product's code
compiled for the host (tests/hostcheck: hc_update_frame, hc_render) against the same oracle, and counts the pixels whose ray has a
direction component of exactly 0 (compute_start_point divides by it: the NaN / Inf paths)."""
import ctypes as C

import numpy as np
import pytest

import raycast_restated as rr

UNIT = np.array([0, 0, 0, 1], np.float32)


# ---- the product's code on the host ------------------------------------------------------------------------------------------
def host_api(hostcheck):
    L = hostcheck.lib
    u8p = np.ctypeslib.ndpointer(np.uint8, flags="C")
    f32p = np.ctypeslib.ndpointer(np.float32, flags="C")
    L.hc_update_frame.argtypes = [f32p, f32p, f32p, f32p, C.c_float, C.c_float, f32p]
    L.hc_render.argtypes = [u8p, C.c_uint32, f32p, C.c_uint32, C.c_uint32, u8p]
    L.hc_render_flags.argtypes = [u8p, C.c_uint32, f32p, C.c_uint32, C.c_uint32, u8p, u8p]
    L.hc_pixel_rays.argtypes = [f32p, C.c_uint32, C.c_uint32, f32p]
    return L


def host_constants(L, bound, eye, vp, w, h):
    cb = np.zeros(22, np.float32)
    assert L.hc_update_frame(np.ascontiguousarray(bound, np.float32), UNIT, eye, np.ascontiguousarray(vp).reshape(-1), w, h, cb) == 0
    return cb


def host_image(L, grid, cb, w, h, empty=None):
    img = np.zeros((h, w, 4), np.uint8)
    g = np.ascontiguousarray(grid).reshape(-1)
    if empty is None:
        L.hc_render(g, grid.shape[0], cb, w, h, img.reshape(-1))
    else:
        L.hc_render_flags(g, grid.shape[0], cb, w, h, np.ascontiguousarray(empty).reshape(-1), img.reshape(-1))
    return img


def zero_direction_pixels(L, cb, w, h):
    """pixels whose ray (pixel_ray of dxv_raycast.h, on the host) has a direction component of exactly 0"""
    rays = np.zeros((h, w, 6), np.float32)
    L.hc_pixel_rays(cb, w, h, rays.reshape(-1))
    return int((rays[..., 3:] == 0).any(-1).sum())


def differing(a, b):
    """(bytes that differ, largest difference, (row, column) of the first differing pixel)"""
    d = a.astype(np.int16) != b.astype(np.int16)
    if not d.any():
        return 0, 0, None
    y, x = np.argwhere(d.any(-1))[0]
    return int(d.sum()), int(np.abs(a.astype(np.int16) - b.astype(np.int16)).max()), (int(y), int(x))


# ---- no GPU needed -----------------------------------------------------------------------------------------------------------
def test_restated_flags_of_hand_made_grids():
    """the restatement itself, against cases worked out by hand"""
    g = np.zeros((16, 16, 16), np.uint8)
    assert rr.brick_flags(g).all() and not rr.brick_summaries(g).any()
    g[8, 8, 8] = 5                                                  # the corner voxel of the last brick: all eight bricks reach it
    assert not rr.brick_flags(g).any()
    assert rr.brick_summaries(g)[1, 1, 1] == 0xFF and rr.brick_summaries(g).sum() == 0xFF
    g[:] = 0
    g[9, 8, 7] = 1                                                  # z = 9, y = 8, x = 7: inside bricks (1, 1, 0); (1, 0, 0) reaches y = 8
    want = np.ones((2, 2, 2), np.uint8)
    want[1, 1, 0] = want[1, 0, 0] = 0
    assert np.array_equal(rr.brick_flags(g), want)
    assert rr.brick_summaries(g)[1, 1, 0] == 0x11 and rr.brick_summaries(g).sum() == 0x11      # any voxel, y = 0 face
    g = np.zeros((10, 10, 10), np.uint8)
    g[9, 9, 9] = 1                                                  # the last voxel of a clipped brick: no other brick reaches it
    want = np.ones((2, 2, 2), np.uint8)
    want[1, 1, 1] = 0
    assert np.array_equal(rr.brick_flags(g), want) and rr.brick_summaries(g)[1, 1, 1] == 0x01
    assert [rr.brick_count(n) for n in rr.SIZES] == [1, 1, 2, 2, 7, 8, 9, 13, 16]
    assert [rr.boundary_brick(n) for n in rr.SIZES] == [None, None, 1, 1, 3, 4, 8, 8, 8]


def test_every_grid_gets_three_cameras_and_an_inside_one():
    for kind in ("dense", "single"):
        for index in range(12):
            names = {name for name, _, _ in rr.views(kind, index)}
            assert len(names) >= 3 and "inside" in names
            assert any(n.startswith("axis") for n in names)
    windows = {(w, h) for kind in ("dense", "single") for _, w, h in rr.views(kind, 0)}
    assert windows == {(1, 1), (17, 33), (160, 90), (161, 91)}
    for N in rr.SIZES:
        n = len(list(rr.written_grids(N)))
        assert n == 12 + 8 + (27 if rr.boundary_brick(N) is not None else 0)


def test_axis_cameras_have_rays_with_a_zero_direction_component(orc, hostcheck, bunny):
    """An eye on a coordinate axis with an odd window: the centre row or column of pixels (the whole of a 1 x 1 window) has a
    direction component of exactly 0 in the product's own arithmetic, so compute_start_point's division by it is exercised by
    every grid of the set.  The other cameras have none."""
    L = host_api(hostcheck)
    _, bound = orc.bound(bunny[0])
    counts = {}
    for name in rr.CAMERAS:
        for w, h in ((1, 1), (17, 33), (33, 19), (161, 91)):
            eye, vp = rr.view_proj(name, bound, w, h)
            counts[name, w, h] = zero_direction_pixels(L, host_constants(L, bound, eye, vp, w, h), w, h)
    for (name, w, h), n in counts.items():
        assert (n >= min(w, h)) if name.startswith("axis") else n == 0, f"{name} {w} x {h}: {n} pixels with a zero direction component; all: {counts}"


@pytest.mark.parametrize("N", rr.SIZES)
def test_host_march_equals_oracle_on_every_grid_and_camera(orc, hostcheck, bunny, N):
    """The CPU half: hc_update_frame + hc_render (the product's dxv_raycast.h compiled for the host) == orc.render for every grid and
    view of the set at small windows; and the host march with the RESTATED flags handed to sample_alpha == the march without."""
    L = host_api(hostcheck)
    vb, ib, _ = bunny
    s = orc.Scene(vb, ib)
    bound = s.bound
    grids = [("dense", "bunny", s.voxelize(N))] + list(rr.written_grids(N))
    bad, zero_rays = [], 0
    for index, (kind, what, grid) in enumerate(grids):
        empty = rr.brick_flags(grid)
        for name, w, h in rr.views(kind, index):
            w, h = rr.small_window(w, h)
            eye, vp = rr.view_proj(name, bound, w, h)
            cb = host_constants(L, bound, eye, vp, w, h)
            zero = zero_direction_pixels(L, cb, w, h)
            zero_rays += zero
            got = host_image(L, grid, cb, w, h)
            want = orc.render(grid, bound, eye, vp, w, h)
            if not np.array_equal(got, want):
                bad.append((what, name, w, h, "host != oracle", differing(got, want), f"{zero} zero-direction pixels"))
            if not np.array_equal(host_image(L, grid, cb, w, h, empty), got):
                bad.append((what, name, w, h, "host with restated flags != host without"))
    assert zero_rays > 0
    assert not bad, f"N = {N}: {len(bad)} views differ ({zero_rays} rays with a zero direction component in the set): {bad[:8]}"


# ---- GPU ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def dxv(dxvlib):
    import dxrvoxelizer_amd
    return dxrvoxelizer_amd


def device_target_image(v, eye, vp, w, h):
    """UpdateFrame + RenderAsync into a torch tensor on the device + Sync"""
    import torch
    t = torch.empty((h, w, 4), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    v.UpdateFrame(0, eye, vp, w, h)
    v.RenderAsync(t)
    v.Sync()
    return t.cpu().numpy()


@pytest.mark.gpu
@pytest.mark.parametrize("N", rr.SIZES)
def test_gpu_display_pass_is_exact_on_every_grid_and_camera(dxv, orc, hostcheck, bunny, N):
    """(a) - (d) of the module docstring for one grid size.  Everything that differs is collected and printed before the one
    assertion, so a failing run shows every figure: bytes that differ, the largest difference, the first differing pixel."""
    from dxrvoxelizer_amd.voxelizer import DBG_BRICK_EMPTY, DBG_BRICK_SUMMARY
    L = host_api(hostcheck)
    vb, ib, _ = bunny
    _, bound = orc.bound(vb)
    v = dxv.Voxelizer(0)
    bad, images = [], 0
    try:
        v.InitFromArrays(vb, ib)
        v.Voxelize(N)
        assert np.allclose(v.stats()["bound"], bound, rtol=0, atol=0)
        for index, (kind, what, grid) in enumerate([("dense", "bunny", None)] + list(rr.written_grids(N))):
            if grid is None:
                grid = v.Grid()
            else:
                rr.write_grid(v, grid)
            for vi, (name, w, h) in enumerate(rr.views(kind, index)):
                eye, vp = rr.view_proj(name, bound, w, h)
                v.set_option("skipempty", 1)
                img = v.Render(eye, vp, w, h)
                if vi == 0:                                            # (a) the flags this render made
                    flags, summary = v.debug(DBG_BRICK_EMPTY), v.debug(DBG_BRICK_SUMMARY)
                    if not np.array_equal(flags, rr.brick_flags(grid)):
                        wrong = np.argwhere(flags != rr.brick_flags(grid))
                        bad.append((what, "flags", len(wrong), "first (bz, by, bx)", wrong[0].tolist(), int(flags[tuple(wrong[0])])))
                    if not np.array_equal(summary, rr.brick_summaries(grid)):
                        wrong = np.argwhere(summary != rr.brick_summaries(grid))
                        bad.append((what, "summaries", len(wrong), "first (bz, by, bx)", wrong[0].tolist(), hex(int(summary[tuple(wrong[0])]))))
                v.set_option("skipempty", 0)
                plain = v.Render(eye, vp, w, h)
                if not np.array_equal(img, plain):                     # (b)
                    bad.append((what, name, w, h, "skipempty 1 != skipempty 0", differing(img, plain)))
                if vi == 0 and kind == "dense":                        # (c)
                    v.set_option("skipempty", 1)
                    if not np.array_equal(device_target_image(v, eye, vp, w, h), img):
                        bad.append((what, name, w, h, "RenderAsync != Render"))
                want = orc.render(grid, bound, eye, vp, w, h)
                images += 1
                if not np.array_equal(img, want):                      # (d)
                    zero = zero_direction_pixels(L, host_constants(L, bound, eye, vp, w, h), w, h)
                    bad.append((what, name, w, h, "device != oracle", differing(img, want), f"{zero} zero-direction pixels"))
        v.set_option("skipempty", 1)
    finally:
        v.close()
    for b in bad:
        print("N = %d:" % N, b)
    assert not bad, f"N = {N}: {len(bad)} of the checks over {images} images failed: {bad[:8]}"


@pytest.mark.gpu
def test_gpu_flags_are_refused_until_a_render_made_them(dxv, bunny):
    from dxrvoxelizer_amd.voxelizer import DBG_BRICK_EMPTY, DBG_BRICK_SUMMARY
    vb, ib, _ = bunny
    bound = None
    v = dxv.Voxelizer(0)
    try:
        v.InitFromArrays(vb, ib)
        v.Voxelize(50)
        bound = v.stats()["bound"]
        eye, vp = rr.view_proj("default", bound, 17, 33)
        for what in (DBG_BRICK_EMPTY, DBG_BRICK_SUMMARY):
            with pytest.raises(dxv.DxvError, match="has not been rendered with empty-brick flags"):
                v.debug(what)
        v.set_option("skipempty", 0)
        v.Render(eye, vp, 17, 33)                                      # a render without flags makes none
        with pytest.raises(dxv.DxvError, match="has not been rendered with empty-brick flags"):
            v.debug(DBG_BRICK_EMPTY)
        v.set_option("skipempty", 1)
        v.Render(eye, vp, 17, 33)
        grid = v.Grid()
        assert np.array_equal(v.debug(DBG_BRICK_EMPTY), rr.brick_flags(grid)) and v.debug(DBG_BRICK_EMPTY).shape == (7, 7, 7)
        buf = np.zeros(7 ** 3 + 1, np.uint8)
        assert v._lib.dxv_debug_download(v._ctx, DBG_BRICK_EMPTY, buf.ctypes.data_as(C.c_void_p), buf.nbytes) == 1
        assert "expected 343 bytes" in v._lib.dxv_last_error(v._ctx).decode()
        v.Voxelize(64)                                                 # another grid size: the flags are the old grid's
        with pytest.raises(dxv.DxvError, match="render it again"):
            v.debug(DBG_BRICK_SUMMARY)
        v.SetFrame(1)                                                  # a frame of its own has none
        v.Voxelize(16)
        with pytest.raises(dxv.DxvError, match="frame 1 has not been rendered"):
            v.debug(DBG_BRICK_EMPTY)
        v.Render(eye, vp, 17, 33)                                      # ... and makes its own on its own stream
        assert np.array_equal(v.debug(DBG_BRICK_EMPTY), rr.brick_flags(v.Grid()))
        assert np.array_equal(v.debug(DBG_BRICK_SUMMARY), rr.brick_summaries(v.Grid()))
    finally:
        v.close()
