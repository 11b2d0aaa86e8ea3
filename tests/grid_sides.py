"""The sides and the grids of the side sweep (tests/test_gpu_grid_sides.py on the device, the *_rule tests through the host-compiled headers):
every grid operator branches on a residue of the side N -- N & 7 picks 8-byte or guarded byte access, N % 64 is the length of a mask row's
last word, N % 8 the tail of a fill column's blocks and the partial 8^3 bricks of the octree, N % 4 the partial 4^3 bricks, N + 1 the cells
of an isosurface row -- so the sweep takes every even side up to 72 and three longer rows.  A plain helper: no fixtures, no hooks."""
import numpy as np

import fill_restated as fr

SWEEP = list(range(2, 73, 2))            # every N % 8 below and above a word; second words of 2, 4, 6, 8 bits; 0..9 fill blocks with tails 0, 2, 4, 6
WIDE = [126, 130, 194]                   # two words, the second of 62 bits; three, the third of 2 bits; four, the fourth of 2 bits

assert {N % 8 for N in SWEEP} == {0, 2, 4, 6}
assert {N % 8 for N in SWEEP if N > 64} == {0, 2, 4, 6}
assert {N % 64 for N in SWEEP + WIDE} >= {2, 4, 6, 8, 62}


def hollow_box(N, lo, hi):
    """a closed shell: the faces of the box [lo, hi]^3"""
    g = np.zeros((N, N, N), np.uint8)
    g[lo:hi + 1, lo:hi + 1, lo:hi + 1] = 1
    g[lo + 1:hi, lo + 1:hi, lo + 1:hi] = 0
    return g


def ends(N):
    """solid on the last valid bit of every other row and on the last slice, next to the bits behind a row's end; bytes other than 1"""
    z, y, x = np.indices((N, N, N))
    g = np.zeros((N, N, N), np.uint8)
    g[(x == N - 1) & ((y + z) % 2 == 0)] = 0x80
    g[(z == N - 1) & (x % 3 == 0)] = 0x02
    return g


def random_grid(N, density):
    return fr.random_walls(N, density, N, bytes_other_than_one=True)


def grids(N, names=None):
    """(name, uint8 [N, N, N]) of the sweep's grids at side N, deterministic; `names` picks some of them"""
    made = {"random 0.6": lambda: random_grid(N, 0.6), "random 0.3": lambda: random_grid(N, 0.3),
            "all 0xFF": lambda: np.full((N, N, N), 0xFF, np.uint8), "ends": lambda: ends(N)}
    if N >= 6:
        made["hollow box"] = lambda: hollow_box(N, 1, N - 2)         # a shell one voxel inside the border: its inside spans every word of a row
    for name in ("random 0.6", "random 0.3", "all 0xFF", "hollow box", "ends"):
        if name in made and (names is None or name in names):
            yield name, made[name]()


WIDE_GRIDS = ("random 0.6", "all 0xFF", "ends")
