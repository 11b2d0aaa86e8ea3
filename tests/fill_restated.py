"""The exterior flood fill restated in numpy, from the rule's text alone (include/dxv.h over dxv_fill_async):

    wall(p)    iff byte(p) != 0
    border(p)  iff any of ix, iy, iz is 0 or N-1
    outside    = the smallest set O with: every p with !wall(p) and border(p) is in O;
                 if p in O, q is one of p's 6 face neighbours inside the grid and !wall(q), then q in O
    SOLID:     byte'(p) = 1 if !outside(p) else 0
    INTERIOR:  byte'(p) = 1 if !outside(p) && !wall(p) else 0

Seed the free border voxels, then repeat R = F & (R | its six shifts) until nothing changes.  No scipy, no sweeps, no bit tricks; the
grids the tests restate are small enough for the diameter of their free space in whole-grid steps."""
import numpy as np

SOLID, INTERIOR = 0, 1


def outside(grid):
    """bool [N, N, N]: the free voxels a 6-connected path of free voxels joins to a free voxel of the grid's border"""
    free = np.asarray(grid) == 0
    reached = np.zeros_like(free)
    for axis in range(3):
        for side in (0, -1):
            idx = [slice(None)] * 3
            idx[axis] = side
            reached[tuple(idx)] = True
    reached &= free
    while True:
        grown = reached.copy()
        grown[1:] |= reached[:-1]
        grown[:-1] |= reached[1:]
        grown[:, 1:] |= reached[:, :-1]
        grown[:, :-1] |= reached[:, 1:]
        grown[:, :, 1:] |= reached[:, :, :-1]
        grown[:, :, :-1] |= reached[:, :, 1:]
        grown &= free
        if np.array_equal(grown, reached):
            return reached
        reached = grown


def fill_from(grid, out, what):
    wall = np.asarray(grid) != 0
    return (~out if what == SOLID else ~out & ~wall).astype(np.uint8)


def fill(grid, what=SOLID):
    """uint8 [N, N, N] of 0 / 1: the filled grid"""
    return fill_from(grid, outside(grid), what)


def maze(N):
    """The baffle maze: every border voxel is wall except (z, y, x) = (1, 0, 1); every even plane y = 2, 4, ... is wall with one
    hole, alternately at (N-2, y, N-2) and (1, y, 1).  One long path, nothing enclosed: the result equals the walls."""
    g = np.zeros((N, N, N), np.uint8)
    g[0] = g[-1] = 1
    g[:, 0] = g[:, -1] = 1
    g[:, :, 0] = g[:, :, -1] = 1
    g[1, 0, 1] = 0
    for k, y in enumerate(range(2, N - 1, 2)):
        g[:, y, :] = 1
        if k % 2 == 0:
            g[N - 2, y, N - 2] = 0
        else:
            g[1, y, 1] = 0
    return g


def random_walls(N, density, seed, bytes_other_than_one=False):
    rng = np.random.default_rng(seed)
    wall = rng.random((N, N, N)) < density
    if bytes_other_than_one:
        return (wall * rng.integers(1, 256, (N, N, N))).astype(np.uint8)
    return wall.astype(np.uint8)
