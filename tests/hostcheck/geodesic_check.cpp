// The product's geodesic routines (csrc/dxv_geodesic.h) compiled for the CPU: the same chain as csrc/geodesic.hip -- the map's first words and the
// live flags of round 0, rounds over the queue of live tiles with double-buffered flags, each tile loaded with its halo into a flat array, relaxed
// until it no longer changes, written back, its neighbours flagged; the tally; the path's descent -- with loops where the device has waves.  A
// round here runs its tiles in index order, one after the other, so a tile sees what the tiles in front of it wrote in the same round: one of
// the orders the device may take.  tests/geodesic_host.py loads this; tests/test_geodesic_rule.py compares it with the two restatements.
#include <stdint.h>
#include <string.h>
#include <vector>
#include "../../dxrvoxelizer_amd/csrc/dxv_geodesic.h"

using namespace dxv;

template <int kMetric> static uint32_t run_rounds(uint32_t* map, uint32_t N, uint32_t limit, std::vector<uint8_t>& live, uint64_t* tilesRun)
{
    const uint32_t side = geo_tiles_side(N), tiles = side * side * side;
    std::vector<uint8_t> next(tiles, 0);
    std::vector<uint32_t> T(kGeoTileWords), was(kGeoTileWords);
    uint32_t rounds = 0;
    for (const uint64_t most = (uint64_t)N * N * N + 2u; rounds < most; ++rounds) {
        std::vector<uint32_t> queue;
        for (uint32_t t = 0; t < tiles; ++t)
            if (live[t]) { queue.push_back(t); live[t] = 0; }
        if (queue.empty()) return rounds + 1u;                          // the confirming round
        *tilesRun += queue.size();
        for (uint32_t tile : queue) {
            const uint32_t tx = tile % side, ty = tile / side % side, tz = tile / (side * side);
            for (uint32_t w = 0; w < kGeoTileWords; ++w) {
                const uint32_t v = geo_tile_voxel(tx, ty, tz, w, N);
                T[w] = v != kGeoNone ? map[v] : kGeoNone;
            }
            was = T;
            if (!geo_relax_tile<kMetric>(T.data(), limit)) continue;
            uint32_t touched = 0;
            for (uint32_t z = 0; z < kGeoTile; ++z)
                for (uint32_t y = 0; y < kGeoTile; ++y)
                    for (uint32_t x = 0; x < kGeoTile; ++x) {
                        const uint32_t at = geo_tile_at(x, y, z);
                        if (T[at] == was[at]) continue;
                        map[geo_tile_voxel(tx, ty, tz, at, N)] = T[at];
                        touched |= geo_touch(x, y, z, kMetric);
                    }
            geo_mark(next.data(), side, tx, ty, tz, touched);
        }
        live.swap(next);
    }
    return 0;                                                           // no fixed point: a bug
}

extern "C" {

// grid: N^3 bytes; seeds: N^3 bytes (GEO_SEEDS_MASK) or seedCount voxel indices (GEO_SEEDS_LIST); map: N^3 uint32, written; tally: {seeds used,
// reached, unreached, farthest, farthest voxel}, written; work: {rounds, tiles run}, written
int gc_geodesic(const uint8_t* grid, uint32_t N, int of, int metric, int kind, const void* seeds, uint32_t seedCount, uint32_t limit, uint32_t* map, uint64_t* tally, uint64_t* work)
{
    if (N < 1u || N > kGeoMaxN || (of != GEO_SOLID && of != GEO_EMPTY) || (metric != GEO_FACES && metric != GEO_CHAMFER) || !geo_fits(N, metric) || kind < GEO_SEEDS_BORDER ||
        kind > GEO_SEEDS_MASK)
        return 1;
    const uint32_t side = geo_tiles_side(N), n3 = N * N * N;
    std::vector<uint8_t> live((size_t)side * side * side, 0);
    const uint8_t* mask = static_cast<const uint8_t*>(seeds);
    const uint32_t* list = static_cast<const uint32_t*>(seeds);
    if (kind != GEO_SEEDS_BORDER && !seeds && (kind == GEO_SEEDS_MASK || seedCount)) return 1;
    if (kind == GEO_SEEDS_LIST)
        for (uint32_t k = 0; k < seedCount; ++k)
            if (list[k] >= n3) return 1;
    for (uint32_t v = 0; v < n3; ++v) {
        const uint32_t row = v / N, x = v - row * N, y = row % N, z = row / N;
        const bool seed = kind == GEO_SEEDS_BORDER ? geo_border(x, y, z, N) : kind == GEO_SEEDS_MASK ? mask[v] != 0 : false;
        map[v] = geo_start(grid[v], of, seed);
        if (!map[v]) geo_mark_seed(live.data(), side, x, y, z);
    }
    if (kind == GEO_SEEDS_LIST)
        for (uint32_t k = 0; k < seedCount; ++k) {
            const uint32_t v = list[k], row = v / N;
            if (map[v] == kGeoNone) continue;
            map[v] = 0u;
            geo_mark_seed(live.data(), side, v - row * N, row % N, row / N);
        }
    work[1] = 0;
    work[0] = metric == GEO_FACES ? run_rounds<GEO_FACES>(map, N, limit, live, work + 1) : run_rounds<GEO_CHAMFER>(map, N, limit, live, work + 1);
    if (!work[0]) return 2;
    GeoTally t{0, 0, 0, 0};
    for (uint32_t first = 0; first < n3; first += 4096u) {              // in pieces, combined: the device's reduction has the same two steps
        GeoTally piece{0, 0, 0, 0};
        for (uint32_t v = first; v < n3 && v < first + 4096u; ++v) geo_tally_voxel(piece, map[v], v);
        geo_tally_combine(t, piece);
    }
    tally[0] = t.seeds; tally[1] = t.reached; tally[2] = t.unreached; tally[3] = geo_tally_farthest(t); tally[4] = geo_tally_farthest_voxel(t);
    return 0;
}

// the path from target down to a seed: 0, or 1 (the target is out of range or holds no distance), 2 (no neighbour continued the path: a bug)
int gc_path(const uint32_t* map, uint32_t N, int metric, uint32_t target, uint32_t* out, uint32_t capacity, uint32_t* length)
{
    if (target >= N * N * N || map[target] >= kGeoUnreached) return 1;
    uint32_t p = target;
    *length = 0;
    for (;;) {
        if (*length < capacity) out[*length] = p;
        ++*length;
        const uint32_t value = map[p], row = p / N;
        if (!value) return 0;
        uint32_t q = kGeoNone;
        for (uint32_t k = 0; k < 27u && q == kGeoNone; ++k) q = geo_descent(map, N, p - row * N, row % N, row / N, k, metric, value);
        if (q == kGeoNone) return 2;
        p = q;
    }
}

uint32_t gc_max_n(void) { return kGeoMaxN; }
uint32_t gc_touch(uint32_t x, uint32_t y, uint32_t z, int metric) { return geo_touch(x, y, z, metric); }
int gc_fits(uint32_t N, int metric) { return geo_fits(N, metric) ? 1 : 0; }

}
