"""The shapes the thinning tests share (tests/test_thin_rule.py on the CPU, tests/test_gpu_thin.py on the device): plain numpy, deterministic,
bytes other than 1 in some of them.  A plain helper: no fixtures, no hooks."""
import numpy as np

import fill_restated as fr
import grid_sides as gs


def full(N):
    return np.full((N, N, N), 0xFF, np.uint8)


def ball(N):
    z, y, x = np.indices((N, N, N))
    c = (N - 1) / 2
    return (((x - c) ** 2 + (y - c) ** 2 + (z - c) ** 2) <= max(0.4 * N, 0.9) ** 2).astype(np.uint8) * 3


def torus(N):
    """round the z axis: ring radius 0.3 N, tube radius 0.12 N -- a solid torus with a hole from side 12 on"""
    z, y, x = np.indices((N, N, N))
    c = (N - 1) / 2
    return (((np.sqrt((x - c) ** 2 + (y - c) ** 2) - 0.3 * N) ** 2 + (z - c) ** 2) <= (0.12 * N) ** 2).astype(np.uint8)


def shell(N):
    """a closed sheet round a cavity: the ball without a smaller ball"""
    z, y, x = np.indices((N, N, N))
    c = (N - 1) / 2
    d = (x - c) ** 2 + (y - c) ** 2 + (z - c) ** 2
    return ((d <= (0.45 * N) ** 2) & (d > (0.25 * N) ** 2)).astype(np.uint8) * 0x80


def plate(N):
    g = np.zeros((N, N, N), np.uint8)
    g[N // 2 - 1:N // 2 + 1, :, :] = 1                                  # two voxels thick, from border to border
    return g


def cross(N):
    """three one-voxel-wide lines through one voxel, each from border to border"""
    g = np.zeros((N, N, N), np.uint8)
    m = N // 2
    g[m, m, :] = g[m, :, m] = g[:, m, m] = 1
    return g


def shapes(N):
    """(name, uint8 [N, N, N]) of every shape at side N, then the grids of the side sweep"""
    for name, make in (("full", full), ("ball", ball), ("torus", torus), ("shell", shell), ("plate", plate), ("cross", cross)):
        yield name, make(N)
    yield "random 0.3 b", fr.random_walls(N, 0.3, 700 + N, bytes_other_than_one=True)
    yield "random 0.6 b", fr.random_walls(N, 0.6, 700 + N, bytes_other_than_one=True)
    yield from gs.grids(N)


def rods(N=130):
    """solid rods three voxels thick along x through bits 62 .. 65 and 126 .. 129 of their rows, one diagonal rod in the xy plane across both word
    boundaries, and a 5 x 5 x 5 block centred on x = 64: candidates at bits 0 and 63 of a word with neighbours in the next one"""
    assert N >= 130
    g = np.zeros((N, N, N), np.uint8)
    g[10:13, 10:13, 62:66] = 1
    g[20:23, 20:23, 126:130] = 0xFF
    for t in range(40, 130):                                            # x = t, y = t - 30: a diagonal three thick in y and z
        g[30:33, t - 31:t - 28, t] = 2
    g[60:65, 60:65, 62:67] = 1
    return g
