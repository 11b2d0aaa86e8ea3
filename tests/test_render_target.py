"""The reference's frame loop (Content/Voxelizer.cpp:81-113, :371-399): UpdateFrame(frameIndex, ...) writes a frame's ray-cast
constants, renderRayCast(frameIndex) draws into a render target on the GPU, three frames are in flight and the host never waits
for an image -- dxv_update_frame, dxv_render_async, dxv_stream_wait_frame (include/dxv.h).  Every image must equal dxv_render's
byte for byte (same kernel, same constants), and dxv_render's is held against the oracle's march."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from dxrvoxelizer_amd import camera

W, H = 1280, 720                     # the reference app's window (Main.cpp:17)
NEW = ("dxv_update_frame", "dxv_render_async", "dxv_stream_wait_frame")


# ---- no GPU needed ---------------------------------------------------------------------------------------------------
def test_new_entry_points_are_exported_and_bound(dxvlib):
    from dxrvoxelizer_amd import _lib
    for name in NEW:
        assert hasattr(dxvlib, name), name
        assert name in _lib.SYMBOLS, name
    assert dxvlib.dxv_api_version() == _lib.API_VERSION == 7


def test_new_entry_points_refuse_a_null_context(dxvlib):
    eye, vp = camera.default_view_proj(W, H)
    eye, vp = np.ascontiguousarray(eye, np.float32), np.ascontiguousarray(vp, np.float32).reshape(16)
    assert dxvlib.dxv_update_frame(None, eye, vp, None, W, H) != 0
    assert dxvlib.dxv_render_async(None, None, W * 4) != 0
    assert dxvlib.dxv_stream_wait_frame(None, None) != 0


def test_raycast_kernels_use_no_scratch(dxvlib):
    from dxrvoxelizer_amd import build
    res = build.kernel_resources("raycast")
    kernels = {k: v for k, v in res.items() if any(n in k for n in ("k_raycast", "k_brick_summary", "k_brick_empty"))}
    assert len(kernels) == 3, sorted(res)
    for k, v in kernels.items():
        assert v["scratch"] == 0, k


# ---- GPU -------------------------------------------------------------------------------------------------------------
def _voxelizer(vb, ib, grid):
    import dxrvoxelizer_amd as dxv
    v = dxv.Voxelizer(0)
    v.InitFromArrays(vb, ib, gridDim=grid)
    return v


def _target(h=H, w=W):
    import torch
    return torch.empty((h, w, 4), dtype=torch.uint8, device="cuda")


def _async_image(v, grid, eye, vp, w=W, h=H, frame=0):
    """UpdateFrame + Voxelize(sync=False) + RenderAsync + Sync: the image of the frame loop"""
    import torch
    t = _target(h, w)
    torch.cuda.synchronize()
    v.UpdateFrame(frame, eye, vp, w, h)
    v.Voxelize(grid, sync=False)
    v.RenderAsync(t)
    v.Sync()
    return t.cpu().numpy()


@pytest.mark.gpu
def test_gpu_render_async_reference_size(dxvlib, orc, bunny):
    """Bunny at 256^3, the app's camera and window: the device target holds dxv_render's image byte for byte, and that is the
    oracle's march byte for byte.  Torus-1M at 512^3 against dxv_render."""
    vb, ib, _ = bunny
    eye, vp = camera.default_view_proj(W, H)
    v = _voxelizer(vb, ib, 256)
    img = _async_image(v, 256, eye, vp)
    st = v.stats()
    assert st["render_ms"] > 0 and st["grid_dim"] == 256
    want = v.Render(eye, vp, W, H)
    assert np.array_equal(img, want)
    _, bound = orc.bound(vb)
    ref = orc.render(v.Grid(), bound, eye, vp, W, H)
    diff = np.abs(img.astype(np.int16) - ref.astype(np.int16))
    assert np.array_equal(img, ref), (int((diff != 0).sum()), int(diff.max()))
    assert 0.05 < (img[..., 3] == 255).mean() < 0.9
    v.close()

    from dxrvoxelizer_amd import meshes
    tvb, tib = meshes.torus()
    v = _voxelizer(tvb, tib, 512)
    img = _async_image(v, 512, eye, vp)
    assert np.array_equal(img, v.Render(eye, vp, W, H))
    assert (img[..., 0] > 100).any()                                # (something of the torus is lit)
    v.close()


@pytest.mark.gpu
def test_gpu_render_async_into_a_pitched_target(dxvlib, bunny):
    """A row slice big[:, :W] of a wider tensor: the image lands in the slice, every padding byte keeps its 0xA5."""
    import torch
    vb, ib, _ = bunny
    eye, vp = camera.default_view_proj(W, H)
    v = _voxelizer(vb, ib, 256)
    big = torch.full((H, W + 37, 4), 0xA5, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()                                        # (the fill is ordered by the caller: the header's rule)
    v.UpdateFrame(0, eye, vp, W, H)
    v.Voxelize(256, sync=False)
    v.RenderAsync(big[:, :W])
    v.Sync()
    got = big.cpu().numpy()
    assert np.array_equal(got[:, :W], v.Render(eye, vp, W, H))
    assert (got[:, W:] == 0xA5).all()
    v.close()


@pytest.mark.gpu
def test_gpu_three_frames_in_flight(dxvlib, bunny):
    """Frames 0 / 1 / 2 with grids 64^3, 100^3, 256^3, three cameras and viewports and their own targets, all enqueued before one
    SyncAll: each image equals a later synchronous dxv_render of that frame.  UpdateFrame on frame 1 leaves frame 0's alone."""
    import torch
    vb, ib, _ = bunny
    v = _voxelizer(vb, ib, 256)
    setups = [(64, 320, 180, camera.DEFAULT_EYE), (100, 200, 120, (-6.0, 3.0, 13.0)), (256, W, H, (0.5, 6.0, -9.0))]
    cams = [camera.default_view_proj(w, h, eye=e) for _, w, h, e in setups]
    targets = [_target(h, w) for _, w, h, _ in setups]
    torch.cuda.synchronize()
    for i, ((n, w, h, _), (eye, vp)) in enumerate(zip(setups, cams)):
        v.UpdateFrame(i, eye, vp, w, h)
        v.Voxelize(n, sync=False, frameIndex=i)
        v.RenderAsync(targets[i])
    v.SyncAll()
    images = [t.cpu().numpy() for t in targets]
    for i, ((n, w, h, _), (eye, vp)) in enumerate(zip(setups, cams)):
        v.SetFrame(i)
        assert v.stats()["grid_dim"] == n
        assert np.array_equal(images[i], v.Render(eye, vp, w, h)), i
    assert not np.array_equal(images[0][:120, :200], images[1])
    # frame 1's new constants are frame 1's only
    eye1, vp1 = camera.default_view_proj(320, 180, eye=(3.0, 1.0, 12.0))
    v.UpdateFrame(1, eye1, vp1, 320, 180)
    again = _target(180, 320)
    torch.cuda.synchronize()
    v.RenderAsync(again, frameIndex=0)
    v.Sync()
    assert np.array_equal(again.cpu().numpy(), images[0])
    v.close()


@pytest.mark.gpu
def test_gpu_lists_frame_has_no_host_round_trip(dxvlib, bunny):
    """A prepared static scene in the reference rule: Voxelize(sync=False) + RenderAsync return while the stream is still busy
    with a spin kernel in front of them -- neither waited for the device."""
    import torch
    vb, ib, _ = bunny
    eye, vp = camera.default_view_proj(W, H)
    v = _voxelizer(vb, ib, 256)
    s = torch.cuda.Stream()
    v.set_stream(s.cuda_stream)
    t = _target()
    torch.cuda.synchronize()
    v.UpdateFrame(0, eye, vp, W, H)
    v.Voxelize(256, sync=False)                                     # warm-up: queue, flags and events exist
    v.RenderAsync(t)
    v.Sync()
    assert v.stats()["list_entries"] > 0
    busy = None
    if hasattr(torch.cuda, "_sleep"):
        torch.cuda._sleep(1000)                                     # (its code object, before the calibration)
        cycles = 1 << 20
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        with torch.cuda.stream(s):
            e0.record(s)
            torch.cuda._sleep(cycles)
            e1.record(s)
        s.synchronize()
        per_ms = cycles / max(e0.elapsed_time(e1), 1e-3)
        cycles = int(min(100.0 * per_ms, 1 << 31))                  # ~100 ms of spinning (at least 50 ms)
        t.zero_()
        torch.cuda.synchronize()
        with torch.cuda.stream(s):
            torch.cuda._sleep(cycles)
        v.Voxelize(256, sync=False)
        v.RenderAsync(t)
        busy = not s.query()
    v.Sync()
    assert np.array_equal(t.cpu().numpy(), v.Render(eye, vp, W, H))
    v.set_stream(None)
    v.close()
    if busy is not None:
        assert busy, "Voxelize(sync=False) + RenderAsync waited for the stream"


@pytest.mark.gpu
def test_gpu_tree_walk_launch_renders_after_host_sync(dxvlib, bunny):
    """lists = 0: the launch walks the tree, its column can run out and be redone -- RenderAsync synchronises first and the image
    is still the right one."""
    vb, ib, _ = bunny
    eye, vp = camera.default_view_proj(W, H)
    v = _voxelizer(vb, ib, 256)
    v.set_option("lists", 0)
    img = _async_image(v, 256, eye, vp)
    assert v.stats()["list_entries"] == 0
    assert np.array_equal(img, v.Render(eye, vp, W, H))
    v.close()


@pytest.mark.gpu
def test_gpu_consumer_stream_waits_on_the_device(dxvlib, bunny):
    """Frame 1 (an internal stream) renders; WaitFrameOn(torch stream) orders a reduction of the target on that stream behind
    the render without a host wait."""
    import torch
    vb, ib, _ = bunny
    eye, vp = camera.default_view_proj(W, H)
    v = _voxelizer(vb, ib, 256)
    t = _target()
    torch.cuda.synchronize()
    v.UpdateFrame(1, eye, vp, W, H)
    v.Voxelize(256, sync=False)
    v.RenderAsync(t)
    s = torch.cuda.Stream()
    v.WaitFrameOn(s)
    with torch.cuda.stream(s):
        total = t.sum(dtype=torch.int64)
    s.synchronize()
    want = v.Render(eye, vp, W, H)
    assert int(total.item()) == int(want.astype(np.int64).sum())
    v.close()


@pytest.mark.gpu
def test_gpu_refusals_launch_nothing(dxvlib, bunny):
    import torch
    import dxrvoxelizer_amd as dxv
    vb, ib, _ = bunny
    eye, vp = camera.default_view_proj(W, H)
    v = _voxelizer(vb, ib, 64)
    t = torch.full((H, W, 4), 0x5A, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    ctx, lib = v._ctx, v._lib
    v.Voxelize(64)
    with pytest.raises(dxv.DxvError, match="dxv_update_frame"):      # no constants yet
        v.RenderAsync(t)
    v.UpdateFrame(0, eye, vp, W, H)
    v.Voxelize(64, z0=0, nz=32)                                     # a slab
    with pytest.raises(dxv.DxvError, match="slab"):
        v.RenderAsync(t)
    v.Voxelize(64)
    assert lib.dxv_render_async(ctx, C.c_void_p(t.data_ptr()), W * 4 - 4) != 0        # pitch below W * 4
    assert lib.dxv_render_async(ctx, C.c_void_p(t.data_ptr()), W * 4 + 2) != 0        # pitch not a multiple of 4
    host = np.zeros((H, W, 4), np.uint8)
    assert lib.dxv_render_async(ctx, host.ctypes.data_as(C.c_void_p), W * 4) != 0      # host memory
    assert "device memory" in lib.dxv_last_error(ctx).decode()
    with pytest.raises(dxv.DxvError, match="singular"):
        v.UpdateFrame(0, eye, np.zeros((4, 4), np.float32), W, H)
    v.Sync()
    assert (t.cpu().numpy() == 0x5A).all()                          # nothing was launched into the target
    # the failed UpdateFrame changed nothing: the frame still renders with the constants it had
    v.RenderAsync(t)
    v.Sync()
    assert np.array_equal(t.cpu().numpy(), v.Render(eye, vp, W, H))
    v.close()


@pytest.mark.gpu
def test_gpu_cpp_render_loop(dxvlib, bunny, tmp_path):
    """tests/cpp/render_loop.cpp over include/dxv_voxelizer.hpp: SetViewport, six frames of UpdateFrame(i % 3) + Render(i % 3, ...)
    into three hipMalloc targets, one wait; the three last images equal dxv_render's."""
    import dxrvoxelizer_amd as dxv
    vb, ib, _ = bunny
    n, w, h = 128, 640, 360
    cams = [camera.default_view_proj(w, h, eye=e) for e in (camera.DEFAULT_EYE, (-6.0, 3.0, 13.0), (0.5, 6.0, -9.0))]
    np.ascontiguousarray(vb, np.float32).tofile(tmp_path / "vb.bin")
    np.ascontiguousarray(ib, np.uint32).tofile(tmp_path / "ib.bin")
    np.concatenate([np.concatenate([np.asarray(e, np.float32), np.asarray(m, np.float32).reshape(16)]) for e, m in cams]).tofile(tmp_path / "cams.bin")
    rocm = "/opt/rocm"
    exe = tmp_path / "render_loop"
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-D__HIP_PLATFORM_AMD__", "-I" + os.path.join(rocm, "include"),
                           os.path.join(ROOT, "tests", "cpp", "render_loop.cpp"), "-o", str(exe),
                           "-L" + os.path.join(ROOT, "dxrvoxelizer_amd"), "-l:libdxv.so", "-L" + os.path.join(rocm, "lib"), "-lamdhip64",
                           "-Wl,-rpath," + os.path.join(ROOT, "dxrvoxelizer_amd"), "-Wl,-rpath," + os.path.join(rocm, "lib")])
    r = subprocess.run([str(exe), str(tmp_path / "vb.bin"), str(tmp_path / "ib.bin"), str(tmp_path / "cams.bin"), str(n), str(w), str(h),
                        str(tmp_path / "img")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    assert int(r.stdout.split()[0]) == n
    v = dxv.Voxelizer(0)
    v.InitFromArrays(vb, ib)
    v.Voxelize(n)
    for i, (eye, vp) in enumerate(cams):
        got = np.fromfile(tmp_path / ("img%d.bin" % i), np.uint8).reshape(h, w, 4)
        assert np.array_equal(got, v.Render(eye, vp, w, h)), i
    v.close()
