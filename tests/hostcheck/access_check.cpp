// The product's access routines (csrc/dxv_access.h) compiled for the CPU: the same chain as csrc/access.hip -- the field of the grid, A's first
// words, the seeds counted and the live flags of round 0, rounds over the queue of live tiles with double-buffered flags, each tile loaded with
// its halo into a flat array, relaxed until nothing rises, written back, its neighbours flagged; the tally; then A into the radius field and
// the thickness's own stages (csrc/dxv_thickness.h) for the intrusion map; the two histograms -- with loops where the device has waves.  A round
// here runs its tiles one after the other, in index order or, with shuffle != 0, in an order shuffled from that seed, so a tile sees what the
// tiles in front of it wrote in the same round: two of the orders the device may take.  tests/access_host.py loads this;
// tests/test_access_rule.py compares it with the restatements.
#include "thickness_check.cpp"
#include "../../dxrvoxelizer_amd/csrc/dxv_access.h"

template <int kConnectivity> static uint32_t acc_run_rounds(uint32_t* A, const int32_t* F, uint32_t N, int of, uint32_t cap, std::vector<uint8_t>& live, uint32_t shuffle, uint64_t* tilesRun)
{
    const uint32_t side = geo_tiles_side(N), tiles = side * side * side;
    std::vector<uint8_t> next(tiles, 0);
    std::vector<uint32_t> T(kGeoTileWords), RT(kGeoTileWords), was(kGeoTileWords);
    uint32_t rounds = 0, state = shuffle;
    for (const uint64_t most = (uint64_t)N * N * N + 2u; rounds < most; ++rounds) {
        std::vector<uint32_t> queue;
        for (uint32_t t = 0; t < tiles; ++t)
            if (live[t]) { queue.push_back(t); live[t] = 0; }
        if (queue.empty()) return rounds + 1u;                          // the confirming round
        if (shuffle)
            for (size_t k = queue.size(); k > 1u; --k) {
                state = state * 1664525u + 1013904223u;
                std::swap(queue[k - 1u], queue[(state >> 8) % k]);
            }
        *tilesRun += queue.size();
        for (uint32_t tile : queue) {
            const uint32_t tx = tile % side, ty = tile / side % side, tz = tile / (side * side);
            for (uint32_t w = 0; w < kGeoTileWords; ++w) {
                const uint32_t v = geo_tile_voxel(tx, ty, tz, w, N);
                T[w] = v != kGeoNone ? A[v] : 0u;
                RT[w] = v != kGeoNone ? thick_radius(F[v], of, cap) : 0u;
            }
            was = T;
            if (!acc_relax_tile<kConnectivity>(T.data(), RT.data())) continue;
            uint32_t touched = 0;
            for (uint32_t z = 0; z < kGeoTile; ++z)
                for (uint32_t y = 0; y < kGeoTile; ++y)
                    for (uint32_t x = 0; x < kGeoTile; ++x) {
                        const uint32_t at = geo_tile_at(x, y, z);
                        if (T[at] == was[at]) continue;
                        A[geo_tile_voxel(tx, ty, tz, at, N)] = T[at];
                        touched |= acc_touch(x, y, z, kConnectivity);
                    }
            geo_mark(next.data(), side, tx, ty, tz, touched);
        }
        live.swap(next);
    }
    return 0;                                                           // no fixed point: a bug
}

// thickness.hip's stages TOP .. HISTOGRAM on a radius field F (tc_thickness's, which makes F of the grid itself)
static int paint_from(const int32_t* F, uint32_t N, int of, uint32_t cap, uint32_t cull, uint32_t* W, uint64_t* hist)
{
    const size_t n3 = (size_t)N * N * N;
    std::vector<int32_t> G(n3);
    std::vector<uint8_t> B(n3);
    for (size_t v = 0; v < n3; ++v) B[v] = thick_radius(F[v], of, cap) == cap;
    field_of(B.data(), N, G.data());
    for (size_t v = 0; v < n3; ++v) {
        B[v] = (uint8_t)thick_top(B[v], G[v], cap);
        W[v] = B[v] ? cap : thick_radius(F[v], of, cap);
    }
    if (cull & THICK_CULL_TOP) field_of(B.data(), N, G.data());
    for (uint32_t z = 0; z < N; ++z)
        for (uint32_t y = 0; y < N; ++y)
            for (uint32_t x = 0; x < N; ++x) {
                const uint32_t items = thick_items(F, G.data(), N, x, y, z, of, cap, cull);
                if (!items) continue;
                const uint32_t R = thick_radius(F[((size_t)z * N + y) * N + x], of, cap), first = thick_disc_first(z, thick_reach(R));
                for (uint32_t k = 0; k < items; ++k)
                    thick_paint_disc(N, x, y, z, R, first + k, 0u, 1u, [&](size_t at, uint32_t r) { if (W[at] < r) W[at] = r; });
            }
    memset(hist, 0, ((size_t)cap + 1u) * sizeof(uint64_t));
    for (size_t v = 0; v < n3; ++v) {
        if (W[v] > cap) return 2;
        ++hist[W[v]];
    }
    return 0;
}

extern "C" {

// grid: N^3 bytes; seeds: N^3 bytes (GEO_SEEDS_MASK) or seedCount voxel indices (GEO_SEEDS_LIST); A, I: N^3 uint32, written (I may be NULL: no
// intrusion map); histA, histI: cap + 1 uint64, written; tally: {seeds used, reached, unreached, widest, widest voxel}, written; work: {rounds,
// tiles run}, written
int ac_access(const uint8_t* grid, uint32_t N, int of, int connectivity, uint32_t cap, int kind, const void* seeds, uint32_t seedCount, uint32_t cull, uint32_t shuffle, uint32_t* A,
              uint32_t* I, uint64_t* histA, uint64_t* histI, uint64_t* tally, uint64_t* work)
{
    if (!acc_valid(N, of, connectivity, cap) || kind < GEO_SEEDS_BORDER || kind > GEO_SEEDS_MASK || cull > 3u) return 1;
    const uint32_t side = geo_tiles_side(N), n3 = N * N * N;
    std::vector<uint8_t> live((size_t)side * side * side, 0);
    const uint8_t* mask = static_cast<const uint8_t*>(seeds);
    const uint32_t* list = static_cast<const uint32_t*>(seeds);
    if (kind != GEO_SEEDS_BORDER && !seeds && (kind == GEO_SEEDS_MASK || seedCount)) return 1;
    if (kind == GEO_SEEDS_LIST)
        for (uint32_t k = 0; k < seedCount; ++k)
            if (list[k] >= n3) return 1;
    std::vector<int32_t> F(n3);
    field_of(grid, N, F.data());
    AccTally t{0, 0, 0, 0};
    for (uint32_t v = 0; v < n3; ++v) {
        const uint32_t row = v / N, x = v - row * N, y = row % N, z = row / N;
        const bool seed = kind == GEO_SEEDS_BORDER ? geo_border(x, y, z, N) : kind == GEO_SEEDS_MASK ? mask[v] != 0 : false;
        A[v] = acc_start(thick_radius(F[v], of, cap), seed);
        if (A[v]) { ++t.seeds; geo_mark_seed(live.data(), side, x, y, z); }
    }
    if (kind == GEO_SEEDS_LIST)
        for (uint32_t k = 0; k < seedCount; ++k) {
            const uint32_t v = list[k], row = v / N, R = thick_radius(F[v], of, cap);
            if (!R) continue;
            if (!A[v]) ++t.seeds;                                       // (a duplicate finds the word raised)
            A[v] = R;
            geo_mark_seed(live.data(), side, v - row * N, row % N, row / N);
        }
    work[1] = 0;
    work[0] = connectivity == 6 ? acc_run_rounds<6>(A, F.data(), N, of, cap, live, shuffle, work + 1) : acc_run_rounds<26>(A, F.data(), N, of, cap, live, shuffle, work + 1);
    if (!work[0]) return 2;
    for (uint32_t first = 0; first < n3; first += 4096u) {              // in pieces, combined: the device's reduction has the same two steps
        AccTally piece{0, 0, 0, 0};
        for (uint32_t v = first; v < n3 && v < first + 4096u; ++v) acc_tally_voxel(piece, A[v], thick_radius(F[v], of, cap), v);
        acc_tally_combine(t, piece);
    }
    tally[0] = t.seeds; tally[1] = t.reached; tally[2] = t.unreached; tally[3] = acc_tally_widest(t); tally[4] = acc_tally_widest_voxel(t);
    memset(histA, 0, ((size_t)cap + 1u) * sizeof(uint64_t));
    for (uint32_t v = 0; v < n3; ++v) {
        if (A[v] > cap) return 2;
        ++histA[A[v]];
    }
    if (!I) return 0;
    for (uint32_t v = 0; v < n3; ++v) F[v] = acc_radius_word(A[v], of);
    return paint_from(F.data(), N, of, cap, cull, I, histI);
}

uint32_t ac_max_n(void) { return kAccMaxN; }
uint32_t ac_touch(uint32_t x, uint32_t y, uint32_t z, int connectivity) { return acc_touch(x, y, z, connectivity); }
int ac_valid(uint32_t N, int of, int connectivity, uint32_t cap) { return acc_valid(N, of, connectivity, cap) ? 1 : 0; }

}
