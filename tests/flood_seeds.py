"""Seeds for the floods (dxv_geodesic, dxv_access) that make one round as wide as the grid: one member voxel out of every 8^3 tile that holds a
member, so round 0 runs every tile at once.  A round is launched with at most 8192 one-wave workgroups (geodesic.hip, access.hip), so from
21 tiles a side -- N = 162: 21^3 = 9261, against 20^3 = 8000 at 160 -- a workgroup takes a second tile in the same launch.  Which member of a
tile is picked varies from tile to tile: seeds lie at corners, on faces and inside tiles, so the neighbour tiles get marked too.  A plain
helper: no fixtures, no hooks."""
import numpy as np

TILE = 8
ROUND_BLOCKS = 8192                                                    # kGeoRoundBlocks, kAccRoundBlocks


def members(g, of):
    """of = 0 (SOLID) the non-zero voxels, 1 (EMPTY) the zero ones, as in every *_restated"""
    return (g != 0) if of == 0 else (g == 0)


def tile_of(idx, N):
    """the 8^3 tile (tz * side + ty) * side + tx of each voxel index (iz * N + iy) * N + ix"""
    idx = np.asarray(idx, np.int64)
    side = (N + TILE - 1) // TILE
    x, y, z = idx % N, idx // N % N, idx // (N * N)
    return (z // TILE * side + y // TILE) * side + x // TILE


def tile_seeds(g, of, k):
    """uint32 voxel indices, ascending by tile: of every 8^3 tile that holds a member of g's kind `of`, its member number h(tile, k) mod (members of
    the tile) in index order -- a multiplicative hash, so the pick differs from tile to tile and from k to k, deterministically"""
    N = g.shape[0]
    idx = np.flatnonzero(members(g, of).reshape(-1))
    tile = tile_of(idx, N)
    order = np.argsort(tile, kind="stable")                             # members by tile, by index inside a tile
    idx, tile = idx[order], tile[order]
    tiles, first, count = np.unique(tile, return_index=True, return_counts=True)
    h = (tiles.astype(np.uint64) * np.uint64(2654435761) + np.uint64(k) * np.uint64(40503) + np.uint64(k)) >> np.uint64(7)
    pick = (h % count.astype(np.uint64)).astype(np.int64)
    return idx[first + pick].astype(np.uint32)


def seed_mask(seeds, N):
    """the same seeds as N^3 bytes, non-zero on a seed (bytes other than 1)"""
    m = np.zeros(N ** 3, np.uint8)
    m[seeds] = 0x40
    return m.reshape(N, N, N)
