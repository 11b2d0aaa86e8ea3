// dxv_geodesic.h -- the geodesic distance inside a grid: with M the members (the solid voxels, or the empty ones) and S the seeds,
//     G(p) = min over paths p0 in S n M, p1, ..., pk = p of allowed steps, of the sum of their weights      (0 on seeds)
// a step from p to q is allowed iff both are members and q is a neighbour of p under the metric: GEO_FACES the 6 face neighbours at weight 1,
// GEO_CHAMFER the 26 neighbours at weight 3 (face), 4 (edge), 5 (corner).  Integer weights: G is the unique least fixed point of
//     G(p) = min(G(p), G(q) + w(q, p))
// so whoever relaxes until nothing changes, in whatever order, ends with the same words.  The routines are here, __host__ __device__:
// geodesic.hip runs them with a wave per 8^3 tile, tests/hostcheck/geodesic_check.cpp serially.
//
// A map word is G(p), or kGeoUnreached on a member no path has reached (yet, or within the limit), or kGeoNone on a voxel that is no member --
// which is also what a tile's halo holds outside the grid: the map itself says who is a member, there is no second mask.
#pragma once
#include <stddef.h>
#include "dxv_types.h"
#include "dxv_scratch.h"

namespace dxv {

enum { GEO_SOLID = 0, GEO_EMPTY = 1 };            // DXV_COMP_SOLID / DXV_COMP_EMPTY
enum { GEO_FACES = 0, GEO_CHAMFER = 1 };          // DXV_GEO_FACES / DXV_GEO_CHAMFER
enum { GEO_SEEDS_BORDER = 0, GEO_SEEDS_LIST = 1, GEO_SEEDS_MASK = 2 };
constexpr uint32_t kGeoNone = 0xFFFFFFFFu, kGeoUnreached = 0xFFFFFFFEu;
constexpr uint32_t kGeoMaxN = 1024;
constexpr uint32_t kGeoTile = 8;                  // a tile is 8^3 voxels ...
constexpr uint32_t kGeoRow = kGeoTile + 2, kGeoPlane = kGeoRow * kGeoRow, kGeoTileWords = kGeoPlane * kGeoRow;   // ... in a flat array of 10^3 words with its halo
constexpr uint32_t kGeoTileVoxels = kGeoTile * kGeoTile * kGeoTile;
constexpr uint32_t kGeoMaxSweeps = kGeoTileVoxels + 1u;       // a relaxation over V voxels with fixed sources settles within V sweeps; one more finds nothing
constexpr uint32_t kGeoMaxRounds = 64;            // rounds of one batch at the most (option georounds); words of the batch's control block
constexpr uint32_t kGeoRoundsDefault = 16;        // ... by default (profiles/NOTES.md, "Geodesic distance")
constexpr uint32_t kGeoSparseTiles = 1024;        // a round with fewer live tiles than this leaves most of the device idle: four one-wave workgroups per CU of 256
constexpr uint32_t kGeoSelf = 13;                 // the slot of the tile itself among the 27 (geo_slot(0, 0, 0))

// the 27 offsets in order of increasing index: dz outermost, dx innermost, each over -1, 0, 1; slot 13 is the voxel itself
DXV_HD uint32_t geo_slot(int dx, int dy, int dz) { return (uint32_t)((dz + 1) * 9 + (dy + 1) * 3 + (dx + 1)); }
DXV_HD int geo_slot_dx(uint32_t k) { return (int)(k % 3u) - 1; }
DXV_HD int geo_slot_dy(uint32_t k) { return (int)(k / 3u % 3u) - 1; }
DXV_HD int geo_slot_dz(uint32_t k) { return (int)(k / 9u) - 1; }
// the weight of the step by (dx, dy, dz), 0 where the metric has no such step
DXV_HD uint32_t geo_weight(int dx, int dy, int dz, int metric)
{
    const uint32_t e2 = (uint32_t)(dx * dx + dy * dy + dz * dz);
    if (metric == GEO_FACES) return e2 == 1u ? 1u : 0u;
    return e2 ? 2u + e2 : 0u;
}
DXV_HD uint32_t geo_max_weight(int metric) { return metric == GEO_FACES ? 1u : 5u; }
DXV_HD uint32_t geo_min_weight(int metric) { return metric == GEO_FACES ? 1u : 3u; }
// no path length can collide with the two codes: wmax (N^3 - 1) < kGeoUnreached
DXV_HD bool geo_fits(uint32_t N, int metric) { return (uint64_t)geo_max_weight(metric) * ((uint64_t)N * N * N - 1u) < (uint64_t)kGeoUnreached; }

DXV_HD bool geo_member(uint32_t byte, int of) { return (byte != 0u) == (of == GEO_SOLID); }
DXV_HD bool geo_border(uint32_t x, uint32_t y, uint32_t z, uint32_t N) { return !x || !y || !z || x == N - 1u || y == N - 1u || z == N - 1u; }
// the map's first word of a voxel
DXV_HD uint32_t geo_start(uint32_t byte, int of, bool seed) { return !geo_member(byte, of) ? kGeoNone : seed ? 0u : kGeoUnreached; }

// One voxel of a tile: T is the flat array, `at` the voxel's place in it (1 .. 8 along every axis), cur = T[at].  What the voxel's word becomes: the
// least of cur and every neighbour's word plus the step's weight; a candidate above the limit (limit != 0) is dropped.
template <int kMetric, class Tile> DXV_HD uint32_t geo_relax(const Tile* T, uint32_t at, uint32_t cur, uint32_t limit)
{
    if (cur == kGeoNone) return cur;
    uint32_t best = cur;
#pragma unroll
    for (int dz = -1; dz <= 1; ++dz)
#pragma unroll
        for (int dy = -1; dy <= 1; ++dy)
#pragma unroll
            for (int dx = -1; dx <= 1; ++dx) {
                const uint32_t w = geo_weight(dx, dy, dz, kMetric);
                if (!w) continue;
                const uint32_t v = T[(int)at + dz * (int)kGeoPlane + dy * (int)kGeoRow + dx];
                if (v < kGeoUnreached && v + w < best && (!limit || v + w <= limit)) best = v + w;
            }
    return best;
}
DXV_HD uint32_t geo_tile_at(uint32_t x, uint32_t y, uint32_t z) { return (z + 1u) * kGeoPlane + (y + 1u) * kGeoRow + (x + 1u); }
// tiles along a side of the grid (the last one partial unless N is a multiple of 8)
DXV_HD uint32_t geo_tiles_side(uint32_t N) { return (N + kGeoTile - 1u) / kGeoTile; }

// word w of the flat array of tile (tx, ty, tz): the voxel of the grid it stands for, kGeoNone outside the grid (an index is below 2^30)
DXV_HD uint32_t geo_tile_voxel(uint32_t tx, uint32_t ty, uint32_t tz, uint32_t w, uint32_t N)
{
    const uint32_t gx = tx * kGeoTile + w % kGeoRow - 1u, gy = ty * kGeoTile + w / kGeoRow % kGeoRow - 1u, gz = tz * kGeoTile + w / kGeoPlane - 1u;
    return gx < N && gy < N && gz < N ? (gz * N + gy) * N + gx : kGeoNone;
}

// The relaxation of one tile, serially: swept until a sweep changes nothing, forwards and backwards in turn so that a front runs through the
// tile in either direction within one sweep.  true: something changed.
template <int kMetric> inline bool geo_relax_tile(uint32_t* T, uint32_t limit)
{
    bool any = false;
    for (uint32_t sweep = 0; sweep < kGeoMaxSweeps; ++sweep) {
        bool changed = false;
        for (uint32_t i = 0; i < kGeoTileVoxels; ++i) {
            const uint32_t k = (sweep & 1u) ? kGeoTileVoxels - 1u - i : i;
            const uint32_t at = geo_tile_at(k % kGeoTile, k / kGeoTile % kGeoTile, k / (kGeoTile * kGeoTile)), v = geo_relax<kMetric>(T, at, T[at], limit);
            if (v != T[at]) { T[at] = v; changed = true; }
        }
        if (!changed) break;
        any = true;
    }
    return any;
}

// A voxel at (x, y, z) of its tile (0 .. 7) changed: the neighbour tiles that hold a neighbour of it under the metric and must therefore run
// again, as bits by geo_slot -- the tiles across the faces it lies on, and under GEO_CHAMFER across its edges and its corner too.
DXV_HD uint32_t geo_touch(uint32_t x, uint32_t y, uint32_t z, int metric)
{
    const int sx = x == 0u ? -1 : x == kGeoTile - 1u ? 1 : 0, sy = y == 0u ? -1 : y == kGeoTile - 1u ? 1 : 0, sz = z == 0u ? -1 : z == kGeoTile - 1u ? 1 : 0;
    uint32_t mask = 0;
#pragma unroll
    for (uint32_t a = 1; a < 8u; ++a) {                                 // a: the axes along which the neighbour tile differs
        if (((a & 1u) && !sx) || ((a & 2u) && !sy) || ((a & 4u) && !sz)) continue;
        const int dx = (a & 1u) ? sx : 0, dy = (a & 2u) ? sy : 0, dz = (a & 4u) ? sz : 0;
        if (geo_weight(dx, dy, dz, metric)) mask |= 1u << geo_slot(dx, dy, dz);
    }
    return mask;
}

// Marks in `live` (a byte per tile, `side` tiles along a side) the tiles of `mask` (bits by geo_slot) round tile (tx, ty, tz) that lie in the grid.
DXV_HD void geo_mark(uint8_t* live, uint32_t side, uint32_t tx, uint32_t ty, uint32_t tz, uint32_t mask)
{
    while (mask) {
        const uint32_t k = (uint32_t)__builtin_ctz(mask);
        mask &= mask - 1u;
        const uint32_t nx = tx + (uint32_t)geo_slot_dx(k), ny = ty + (uint32_t)geo_slot_dy(k), nz = tz + (uint32_t)geo_slot_dz(k);
        if (nx < side && ny < side && nz < side) live[(nz * side + ny) * side + nx] = 1;
    }
}
// A seed at voxel (x, y, z) of the grid: its own tile runs in round 0, and so does every tile that holds a neighbour of it -- a seed's word never
// changes, so no round would flag them (under either metric: the face tiles relax nothing new under GEO_FACES and settle at once).
DXV_HD void geo_mark_seed(uint8_t* live, uint32_t side, uint32_t x, uint32_t y, uint32_t z)
{
    geo_mark(live, side, x / kGeoTile, y / kGeoTile, z / kGeoTile, 1u << kGeoSelf | geo_touch(x % kGeoTile, y % kGeoTile, z % kGeoTile, GEO_CHAMFER));
}

// The path's descent: the neighbour of (x, y, z) in slot k when it lies in the grid, is a neighbour under the metric and its word plus the step's
// weight is `value`, the word of (x, y, z); kGeoNone otherwise.  The path takes the first such slot.
DXV_HD uint32_t geo_descent(const uint32_t* map, uint32_t N, uint32_t x, uint32_t y, uint32_t z, uint32_t k, int metric, uint32_t value)
{
    const int dx = geo_slot_dx(k), dy = geo_slot_dy(k), dz = geo_slot_dz(k);
    const uint32_t w = geo_weight(dx, dy, dz, metric);
    const uint32_t qx = x + (uint32_t)dx, qy = y + (uint32_t)dy, qz = z + (uint32_t)dz;
    if (!w || qx >= N || qy >= N || qz >= N) return kGeoNone;
    const uint32_t q = (qz * N + qy) * N + qx, v = map[q];
    return v < kGeoUnreached && v + w == value ? q : kGeoNone;
}

// The tally: seeds used (the words that are 0: only a seed's is), members reached and unreached, and the greatest word with the smallest index
// that holds it as one key -- the word above, the index's complement below, so that the greater key is the farther voxel or the earlier one.
// Sums and a maximum of integers: the order of the combines does not matter.
struct GeoTally { unsigned long long seeds, reached, unreached, key; };
DXV_HD void geo_tally_voxel(GeoTally& t, uint32_t word, uint32_t index)
{
    if (word == kGeoNone) return;
    if (word == kGeoUnreached) { ++t.unreached; return; }
    ++t.reached;
    if (!word) ++t.seeds;
    const unsigned long long key = (unsigned long long)word << 32 | (0xFFFFFFFFu - index);
    if (key > t.key) t.key = key;
}
DXV_HD void geo_tally_combine(GeoTally& a, const GeoTally& b)
{
    a.seeds += b.seeds; a.reached += b.reached; a.unreached += b.unreached;
    if (b.key > a.key) a.key = b.key;
}
// nothing reached: key 0 reads farthest 0 at voxel 0xFFFFFFFF
DXV_HD uint32_t geo_tally_farthest(const GeoTally& t) { return (uint32_t)(t.key >> 32); }
DXV_HD uint32_t geo_tally_farthest_voxel(const GeoTally& t) { return 0xFFFFFFFFu - (uint32_t)(t.key & 0xFFFFFFFFu); }

// ---- scratch of a flood in tiles (geodesic.hip, access.hip) ----
// the batch's control block -- word k = the live tiles of round k; the batch has reached the fixed point exactly when one of its words is 0 --
// and the tally behind the rounds: {seeds used, reached, unreached, the operator's own key}
struct GeoControl {
    uint32_t live[64];                // (kGeoMaxRounds)
    unsigned long long tally[4];      // GeoTally
};
inline uint32_t geo_tiles(uint32_t N) { return geo_tiles_side(N) * geo_tiles_side(N) * geo_tiles_side(N); }
// the control block, two sets of live flags (a byte per 8^3 tile; flagBytes: both, cleared together) and the queue (a word per tile)
struct GeoScratch { GeoControl* ctl; uint8_t* flags[2]; size_t flagBytes; uint32_t* queue; };
inline void geodesic_carve(Carve& c, uint32_t N, GeoScratch& l)
{
    l.ctl = c.take<GeoControl>(1);
    const size_t from = c.used();
    l.flags[0] = c.take<uint8_t>(geo_tiles(N));
    l.flags[1] = c.take<uint8_t>(geo_tiles(N));
    l.flagBytes = c.used() - from;
    l.queue = c.take<uint32_t>(geo_tiles(N));
}
inline size_t geodesic_scratch_bytes(uint32_t N) { return carved_bytes<GeoScratch>(geodesic_carve, N); }

} // namespace dxv
