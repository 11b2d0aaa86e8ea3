"""The display pass and the frame loop at the reference's window (1280 x 720, Main.cpp:17).  One JSON line per case:

  render    render_ms (empty-brick flags + ray-cast, the frame's device events) per mesh / grid, option skipempty on and off, and
            the two apart: flag_pass_ms = the render of a 1 x 1 viewport whose one ray points away from the volume (the flags and
            a ray-cast that ends at once), raycast_ms = the rest (skipempty 1)
  loop      frames per second over 200 frames of a scene prepared by Init(gridDim):
              a: Voxelize (synchronous) + dxv_render to the host, every frame;
              b: Voxelize(sync=False) + RenderAsync into three device targets, three frames in flight, one SyncAll at the end

usage: render_times.py [--quick]   (--quick: bunny 64^3 only, 20 frames: a rehearsal of the script)"""
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import dxrvoxelizer_amd as dxv  # noqa: E402
from bench import make_mesh  # noqa: E402
from dxrvoxelizer_amd import camera  # noqa: E402

W, H = 1280, 720


def render_ms(v, grid, frame=0, reps=20, w=W, h=H, away=False):
    """median render_ms of RenderAsync + Sync of the frame's constants for a w x h target; away: the camera looks away from the
    volume (its rays end at once: what is left is the flag pass)"""
    import torch
    t = torch.empty((h, w, 4), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    eye, vp = camera.default_view_proj(w, h, eye=(0.0, 4.0, -60.0), focus=(0.0, 4.0, -120.0)) if away else camera.default_view_proj(w, h)
    v.UpdateFrame(frame, eye, vp, w, h)
    out = []
    for i in range(3 + reps):
        v.RenderAsync(t)
        v.Sync()
        if i >= 3:
            out.append(v.stats()["render_ms"])
    return statistics.median(out)


def loop_a(v, grid, frames):
    eye, vp = camera.default_view_proj(W, H)
    v.SetFrame(0)
    for _ in range(3):
        v.Voxelize(grid)
        v.Render(eye, vp, W, H)
    t0 = time.perf_counter()
    for _ in range(frames):
        v.Voxelize(grid)
        v.Render(eye, vp, W, H)
    return frames / (time.perf_counter() - t0)


def loop_b(v, grid, frames):
    import torch
    targets = [torch.empty((H, W, 4), dtype=torch.uint8, device="cuda") for _ in range(v.FrameCount)]
    torch.cuda.synchronize()
    for f in range(v.FrameCount):
        eye, vp = camera.default_view_proj(W, H, eye=(8.0 - 2.0 * f, 12.0, -14.0))
        v.UpdateFrame(f, eye, vp, W, H)

    def run(n):
        for i in range(n):
            f = i % v.FrameCount
            v.Voxelize(grid, sync=False, frameIndex=f)
            v.RenderAsync(targets[f])
        v.SyncAll()

    run(6)
    t0 = time.perf_counter()
    run(frames)
    return frames / (time.perf_counter() - t0)


def main():
    import torch
    torch.cuda.init()                        # (torch's device before the library's first context, as bench.py does)
    quick = "--quick" in sys.argv
    cases = [("bunny", 64)] if quick else [("bunny", 64), ("torus1m", 256), ("torus1m", 512), ("dragon9", 512)]
    frames = 20 if quick else 200
    meshes = {}
    for k, (name, grid) in enumerate(cases):
        if name not in meshes:
            meshes[name] = make_mesh(name)
        vb, ib, label = meshes[name]
        v = dxv.Voxelizer(0)
        v.InitFromArrays(vb, ib, gridDim=grid)
        v.SetFrame(0)
        v.Voxelize(grid)
        if k == 0:
            render_ms(v, grid, reps=300)                                 # (the process's first case: clocks up before anything is timed)
        row = {"case": "render", "mesh": label, "grid": grid, "width": W, "height": H}
        for skip in (1, 0):
            v.set_option("skipempty", skip)
            row["render_ms_skipempty%d" % skip] = round(render_ms(v, grid), 4)
        v.set_option("skipempty", 1)
        flags = render_ms(v, grid, w=1, h=1, away=True)
        row["flag_pass_ms"] = round(flags, 4)
        row["raycast_ms"] = round(row["render_ms_skipempty1"] - flags, 4)
        v.Voxelize(grid)
        row["voxelize_ms"] = round(v.stats()["voxelize_ms"], 4)
        print(json.dumps(row), flush=True)
        fa, fb = loop_a(v, grid, frames), loop_b(v, grid, frames)
        print(json.dumps({"case": "loop", "mesh": label, "grid": grid, "width": W, "height": H, "frames": frames,
                          "fps_a_sync_host": round(fa, 1), "fps_b_async_device": round(fb, 1), "b_over_a": round(fb / fa, 3)}), flush=True)
        v.close()


if __name__ == "__main__":
    main()
