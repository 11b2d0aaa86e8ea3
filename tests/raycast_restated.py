"""The display pass's empty-brick flags restated in numpy, and the adversarial grids and cameras the display pass is held to
(tests/test_raycast_exact.py).

Flags -- from the comment over sample_alpha in dxrvoxelizer_amd/csrc/dxv_raycast.h, not from the kernels: one byte per 8 x 8 x 8
brick, 1 where the voxels [8b, 8b+8] per axis (the brick and the first plane of its +x / +y / +z neighbours, clipped to the grid)
are all 0.  Summaries -- from the comment over k_brick_summary in raycast.hip: eight bits per brick about the brick's own voxels.
The image has no restatement here: its reference is the oracle's march (oracle/orc.py render)."""
import itertools

import numpy as np

from dxrvoxelizer_amd import camera

BRICK = 8

# ---- the flags ---------------------------------------------------------------------------------------------------------------
def brick_count(N):
    return (N + BRICK - 1) // BRICK


def brick_flags(grid):
    """empty[bz, by, bx] = not grid[8bz : 8bz+9, 8by : 8by+9, 8bx : 8bx+9].any()   (numpy clips the slices to N)"""
    N = grid.shape[0]
    M = brick_count(N)
    empty = np.zeros((M, M, M), np.uint8)
    for bz, by, bx in itertools.product(range(M), repeat=3):
        empty[bz, by, bx] = not grid[8 * bz:8 * bz + 9, 8 * by:8 * by + 9, 8 * bx:8 * bx + 9].any()
    return empty


def brick_summaries(grid):
    """bit0 any voxel of the brick, bit1 any on its x=0 face, bit2 z=0 face, bit3 x=0,z=0 edge, bit4 y=0 face, bit5 x=0,y=0 edge,
    bit6 y=0,z=0 edge, bit7 the corner voxel -- of the brick's own 8^3 voxels (those inside the grid)"""
    N = grid.shape[0]
    M = brick_count(N)
    out = np.zeros((M, M, M), np.uint8)
    for bz, by, bx in itertools.product(range(M), repeat=3):
        b = grid[8 * bz:8 * bz + 8, 8 * by:8 * by + 8, 8 * bx:8 * bx + 8] != 0              # [z, y, x]; never empty: 8b < N
        bits = (b.any(), b[:, :, 0].any(), b[0].any(), b[0, :, 0].any(), b[:, 0].any(), b[:, 0, 0].any(), b[0, 0].any(), b[0, 0, 0])
        out[bz, by, bx] = sum(int(bool(v)) << k for k, v in enumerate(bits))
    return out


# ---- grids -------------------------------------------------------------------------------------------------------------------
SIZES = (2, 8, 10, 16, 50, 64, 72, 100, 128)     # 64-bit row load (N % 8 == 0) and byte loop; M = 1, 1, 2, 2, 7, 8, 9, 13, 16


def write_grid(v, grid):
    """overwrite the selected frame's grid through dxv_grid_device_ptr, the way tests/test_gpu_prepared.py poisons it"""
    import torch
    from dxrvoxelizer_amd.slabs import device_grid_tensor
    v.Sync()
    t = device_grid_tensor(v, "cuda")
    assert t.numel() == grid.size
    t.copy_(torch.from_numpy(np.ascontiguousarray(grid, np.uint8).reshape(-1)))
    torch.cuda.synchronize()


def boundary_brick(N):
    """the k of the single-voxel grids: brick boundary 8k with 8k + 1 < N, the first brick of the second run of eight where the
    grid has one (M > 8), else the middle one; None where the grid has no interior brick boundary (N <= 9)"""
    M = brick_count(N)
    k = 8 if M > 8 else M // 2
    return k if k >= 1 and 8 * k + 1 < N else None


def single_voxel_grids(N):
    """("kind", name, grid): one voxel at every combination of {8k-1, 8k, 8k+1} per axis, then one at each corner of the grid"""
    k = boundary_brick(N)
    if k is not None:
        for dz, dy, dx in itertools.product((-1, 0, 1), repeat=3):
            g = np.zeros((N, N, N), np.uint8)
            g[8 * k + dz, 8 * k + dy, 8 * k + dx] = 1
            yield "single", f"voxel at brick {k} {dz:+d}{dy:+d}{dx:+d}", g
    for cz, cy, cx in itertools.product((0, N - 1), repeat=3):
        g = np.zeros((N, N, N), np.uint8)
        g[cz, cy, cx] = 0x80
        yield "single", f"corner voxel {cz},{cy},{cx}", g


def dense_grids(N):
    rng = np.random.default_rng(1000 + N)
    z, y, x = np.indices((N, N, N))
    yield "dense", "all zero", np.zeros((N, N, N), np.uint8)
    yield "dense", "all 0xFF", np.full((N, N, N), 0xFF, np.uint8)
    for density in (0.5, 1e-2, 1e-4):
        g = ((rng.random((N, N, N)) < density) * rng.integers(1, 256, (N, N, N))).astype(np.uint8)      # (any byte but 0 is solid)
        if not g.any():
            g[N // 3, N // 2, N - 1] = 0x80
        yield "dense", f"random {density}", g
    yield "dense", "checkerboard", ((x + y + z) & 1).astype(np.uint8)
    for axis, side in itertools.product(range(3), (0, N - 1)):
        g = np.zeros((N, N, N), np.uint8)
        idx = [slice(None)] * 3
        idx[axis] = side
        g[tuple(idx)] = 1 + axis
        yield "dense", f"slab axis {axis} at {side}", g


def written_grids(N):
    """every grid of size N that is written through the grid pointer (the bunny's own grid at N comes from the voxelizer)"""
    yield from dense_grids(N)
    yield from single_voxel_grids(N)


# ---- cameras -----------------------------------------------------------------------------------------------------------------
# name -> (eye, focus, up); "local" ones are in the cube's space [-1, 1]^3 (world = centre + half extent * local)
CAMERAS = {
    "default": ("world", camera.DEFAULT_EYE, camera.DEFAULT_FOCUS, (0, 1, 0)),          # the app's start-up camera
    "oblique": ("world", (-6.0, 3.0, 13.0), camera.DEFAULT_FOCUS, (0, 1, 0)),
    "inside": ("local", (0.3, -0.2, 0.45), (-0.5, 0.1, -0.7), (0, 1, 0)),               # eye inside the cube (inside solid in the all-0xFF grid)
    "inside corner": ("local", (0.9, 0.9, -0.9), (-1.0, -1.0, 1.0), (0, 1, 0)),         # ... near a corner, looking along the diagonal
    "far": ("local", (150.0, 120.0, -180.0), (0.0, 0.0, 0.0), (0, 1, 0)),               # the cube a few pixels wide
    # an eye on each coordinate axis looking at the centre: the centre row / column of an odd window has direction components of
    # exactly 0 (compute_start_point divides by them) -- how many is counted on the CPU, tests/test_raycast_exact.py
    "axis +x": ("local", (4.0, 0.0, 0.0), (0.0, 0.0, 0.0), (0, 1, 0)),
    "axis -x": ("local", (-4.0, 0.0, 0.0), (0.0, 0.0, 0.0), (0, 1, 0)),
    "axis +y": ("local", (0.0, 4.0, 0.0), (0.0, 0.0, 0.0), (0, 0, 1)),
    "axis -y": ("local", (0.0, -4.0, 0.0), (0.0, 0.0, 0.0), (0, 0, 1)),
    "axis +z": ("local", (0.0, 0.0, 4.0), (0.0, 0.0, 0.0), (0, 1, 0)),
    "axis -z": ("local", (0.0, 0.0, -4.0), (0.0, 0.0, 0.0), (0, 1, 0)),
}
AXES = tuple(n for n in CAMERAS if n.startswith("axis"))


def view_proj(name, bound, width, height):
    """(eye, view @ proj) of a named camera for a mesh bound (centre.xyz, half extent) and a window"""
    space, eye, focus, up = CAMERAS[name]
    eye, focus = np.asarray(eye, np.float64), np.asarray(focus, np.float64)
    if space == "local":
        c, w = np.asarray(bound[:3], np.float64), float(bound[3])
        eye, focus = c + w * eye, c + w * focus
    vp = camera.look_at_lh(eye, focus, up) @ camera.perspective_fov_lh(camera.FOV_Y, width / height, camera.Z_NEAR, camera.Z_FAR)
    return eye.astype(np.float32), vp.astype(np.float32)


def views(kind, index):
    """the (camera, width, height) a grid is rendered with: `kind` "dense" (and the bunny) or "single", `index` its place among the
    grids of its size (deals the six axis cameras round).  Every grid: at least three cameras, an inside one among them."""
    axis = AXES[index % len(AXES)]
    if kind == "single":
        return [("default", 17, 33), ("inside", 17, 33), (axis, 161, 91)]
    return [("default", 160, 90), ("oblique", 17, 33), ("inside", 161, 91), ("inside corner", 17, 33), (axis, 161, 91),
            (AXES[(index + 3) % len(AXES)], 17, 33), ("far", 17, 33), ("default", 1, 1), (axis, 1, 1)]


def small_window(width, height):
    """the window of the same view in the CPU half: the large ones shrunk, odd stays odd (a centre pixel exists)"""
    return {(160, 90): (32, 18), (161, 91): (33, 19)}.get((width, height), (width, height))
