"""The second trip of the floods' tile loop: k_geo_round and k_acc_round are launched with at most 8192 one-wave workgroups, and a workgroup
takes a second tile only when one round has more live tiles than that -- at least 21 tiles a side (N >= 162) with seeds in more than 8192 of
them at once.  What makes the second trip right is the loop's own code: `touched` reset, the barrier before the next tile's load overwrites the
tile in LDS, the lane's eight words (and radii) reloaded per tile.  The border marks 25^3 - 23^3 = 3458 tiles at side 194 and a single voxel's
front is a shell, so the sweeps (test_gpu_geodesic_sides.py, test_gpu_access_sides.py) never get there.  Here one member of every 8^3 tile is a
seed (tests/flood_seeds.py) of "random 0.3" at side 162 (21^3 = 9261 tiles, 162 % 8 = 2: the last tile of every row is partial), both kinds:
round 0 runs all 9261 tiles.  Each test asserts that first -- in numpy on the seeds, and from the device's own work info after the call --, then
compares maps, histograms and tally as bytes with the host libraries (tests/geodesic_host.py, tests/access_host.py; the *_rule tests hold them
to the restatements with this seeding).  The seeds go in as a list (k_geo_seed_list, k_acc_seed_list) and as a mask on the device (k_geo_init,
k_acc_init): the same bytes.  One case of each operator runs with one round per batch, so round 0 is a launch settled on its own.  Side 160
(20^3 = 8000 tiles: one trip) with the same seeding tells the second trip from the seeding when 162 fails.
Host library at 162, per call: geodesic 1.9 .. 4.6 s (FACES / CHAMFER: solid 1.9 / 2.4 s, empty 2.7 / 4.6 s), access 0.8 .. 1.5 s with the
intrusion map; at 160 geodesic solid FACES 2.0 s, access solid 6 2.5 s.  One item is one kind and one metric or connectivity."""
import functools

import numpy as np
import pytest

import access_host as ah
import access_restated as ar
import flood_seeds as fs
import geodesic_host as gh
import geodesic_restated as gr
import grid_sides as gs
from raycast_restated import write_grid

pytestmark = pytest.mark.gpu
GEO_TALLY = ("seeds_used", "reached", "unreached", "farthest", "farthest_voxel")
ACC_TALLY = ("seeds_used", "reached", "unreached", "widest", "widest_voxel")
CAP = 65
TWO_TRIPS, ONE_TRIP = 162, 160


@pytest.fixture(scope="module")
def writer(dxvlib, bunny):
    """the one Voxelizer, on the bunny, whose frame every grid of this file is written into"""
    import dxrvoxelizer_amd
    vb, ib, _ = bunny
    v = dxrvoxelizer_amd.Voxelizer(0)
    v.InitFromArrays(vb, ib)
    yield v
    v.close()


@functools.lru_cache(maxsize=None)
def grid(N):
    return dict(gs.grids(N, ("random 0.3",)))["random 0.3"]


def load(v, N):
    """the frame holds "random 0.3" of side N"""
    if v.stats()["grid_dim"] != N:
        v.Voxelize(N)
    write_grid(v, grid(N))
    return grid(N)


def seeds_of(g, of, k):
    """(list, mask on the device, tiles of the grid) of the per-tile seeding, which puts a seed into every tile"""
    import torch
    N = g.shape[0]
    seeds = fs.tile_seeds(g, of, k)
    tiles = ((N + 7) // 8) ** 3
    assert fs.members(g, of).reshape(-1)[seeds].all() and len(np.unique(seeds)) == len(seeds)
    assert len(np.unique(fs.tile_of(seeds, N))) == len(seeds) == tiles
    assert {int(s) % 8 for s in seeds % N} == set(range(8))             # corners, faces and insides of tiles
    return seeds, torch.from_numpy(fs.seed_mask(seeds, N)).cuda(), tiles


def check_geodesic(v, g, of, metric, seeds, want, tally, tiles, what):
    got = v.Geodesic(of, metric, seeds)
    work, info = v.geodesic_work_info(), v.GeodesicInfo()
    assert work["most_live_tiles"] == tiles, (what, work)
    assert (work["most_live_tiles"] > fs.ROUND_BLOCKS) == (g.shape[0] == TWO_TRIPS), (what, work)
    assert got.dtype == want.dtype and got.shape == want.shape and got.tobytes() == want.tobytes(), what
    assert {k: info[k] for k in GEO_TALLY} == tally, what
    return info


def check_access(v, g, of, connectivity, seeds, want, tiles, what, intrusion=True):
    A, I = v.Access(of, connectivity, CAP, seeds, intrusion=intrusion)
    work, info = v.access_work_info(), v.AccessInfo()
    assert work["most_live_tiles"] == tiles, (what, work)
    assert (work["most_live_tiles"] > fs.ROUND_BLOCKS) == (g.shape[0] == TWO_TRIPS), (what, work)
    assert A.dtype == want["A"].dtype and A.shape == want["A"].shape and A.tobytes() == want["A"].tobytes(), what
    assert v.AccessHistogram().tobytes() == want["hist_a"].tobytes(), what
    if intrusion:
        assert I.tobytes() == want["I"].tobytes() and v.IntrusionHistogram().tobytes() == want["hist_i"].tobytes(), what
    else:
        assert I is None, what
    assert {k: info[k] for k in ACC_TALLY} == want["tally"], what
    return info


@pytest.mark.parametrize("metric", [gr.FACES, gr.CHAMFER])
@pytest.mark.parametrize("of", [gr.SOLID, gr.EMPTY])
def test_geodesic_with_every_tile_live_in_round_0(writer, of, metric):
    v = writer
    g = load(v, TWO_TRIPS)
    seeds, mask, tiles = seeds_of(g, of, 1 + metric)
    assert tiles == 9261 > fs.ROUND_BLOCKS
    want, tally, _ = gh.geodesic(g, of, metric, seeds)
    assert tally["seeds_used"] == tiles
    check_geodesic(v, g, of, metric, seeds, want, tally, tiles, ("list", of, metric))
    check_geodesic(v, g, of, metric, mask, want, tally, tiles, ("mask", of, metric))
    if (of, metric) == (gr.SOLID, gr.FACES):                            # every round settled on the host: round 0 is a launch of 9261 tiles on its own
        try:
            v.set_option("georounds", 1)
            info = check_geodesic(v, g, of, metric, seeds, want, tally, tiles, ("georounds 1", of, metric))
            assert info["rounds"] > 2
        finally:
            v.set_option("georounds", 0)


@pytest.mark.parametrize("connectivity", [6, 26])
@pytest.mark.parametrize("of", [ar.SOLID, ar.EMPTY])
def test_access_with_every_tile_live_in_round_0(writer, of, connectivity):
    v = writer
    g = load(v, TWO_TRIPS)
    seeds, mask, tiles = seeds_of(g, of, 3 + connectivity)
    assert tiles == 9261 > fs.ROUND_BLOCKS
    want = ah.access(g, of, connectivity, CAP, seeds)
    assert want["tally"]["seeds_used"] == tiles
    check_access(v, g, of, connectivity, seeds, want, tiles, ("list", of, connectivity))
    check_access(v, g, of, connectivity, mask, want, tiles, ("mask", of, connectivity))
    check_access(v, g, of, connectivity, seeds if connectivity == 6 else mask, want, tiles, ("no intrusion map", of, connectivity), intrusion=False)
    if (of, connectivity) == (ar.SOLID, 26):                            # every round settled on the host: round 0 is a launch of 9261 tiles on its own
        try:
            v.set_option("accessrounds", 1)
            info = check_access(v, g, of, connectivity, seeds, want, tiles, ("accessrounds 1", of, connectivity))
            assert info["rounds"] > 2
        finally:
            v.set_option("accessrounds", 0)


def test_one_trip_at_side_160_with_the_same_seeding(writer):
    v = writer
    g = load(v, ONE_TRIP)
    seeds, mask, tiles = seeds_of(g, gr.SOLID, 1)
    assert tiles == 8000 <= fs.ROUND_BLOCKS
    want, tally, _ = gh.geodesic(g, gr.SOLID, gr.FACES, seeds)
    check_geodesic(v, g, gr.SOLID, gr.FACES, seeds, want, tally, tiles, ("list", 160))
    check_geodesic(v, g, gr.SOLID, gr.FACES, mask, want, tally, tiles, ("mask", 160))
    want = ah.access(g, ar.SOLID, 6, CAP, seeds)
    check_access(v, g, ar.SOLID, 6, seeds, want, tiles, ("list", 160))
    check_access(v, g, ar.SOLID, 6, mask, want, tiles, ("mask", 160))
