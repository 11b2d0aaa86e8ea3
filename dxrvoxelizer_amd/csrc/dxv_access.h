// dxv_access.h -- the access radius inside a grid and its intrusion map: with M the members (the solid voxels, or the empty ones),
// S the seeds and R(c) = min(D2(c), cap_sq) dxv_thickness's radius (0 off the members),
//     A(c) = max over paths p0 in S n M, p1, ..., pk = c of members, consecutive voxels adjacent under the connectivity, of min R(pi)   (0: no path, no member)
//     I(p) = max { A(c) : c in M, |p - c|^2 < A(c) }       for p in M, 0 elsewhere and where the set is empty
// Integers only.  A is the least fixed point, from the start word below, of
//     A(c) = max(A(c), min(R(c), max over the neighbours q of A(q)))
// and every step of it is monotone, so whoever relaxes until nothing rises, in whatever order, ends with the same words.  I is dxv_thickness's
// paint with A for R (thick_radius's encoding): a set function of A.  The routines are here, __host__ __device__: access.hip runs them with a wave
// per 8^3 tile, tests/hostcheck/access_check.cpp serially.  The tiles, their halo, the slots and the live flags are dxv_geodesic.h's.
//
// A map word is A(c): 0 on a voxel that is no member, on a member no path has reached, and in a tile's halo outside the grid -- a 0 raises
// nothing, so the map and R together say everything (R > 0 exactly on the members: the tally tells "no member" from "not reached").
#pragma once
#include "dxv_geodesic.h"
#include "dxv_thickness.h"

namespace dxv {

constexpr uint32_t kAccMaxN = kThickMaxN;
constexpr uint32_t kAccMaxSweeps = kGeoTileVoxels + 1u;       // of the words of a tile that are not final, the highest whose path predecessor is final becomes final in the next sweep
constexpr uint32_t kAccMaxRounds = kGeoMaxRounds;  // rounds of one batch at the most (option accessrounds); words of the batch's control block
constexpr uint32_t kAccRoundsDefault = kGeoRoundsDefault;

// 6: the face neighbours, 26: faces, edges and corners (dxv_components' adjacency) -- as the metric whose steps they are
DXV_HD bool acc_connectivity(int connectivity) { return connectivity == 6 || connectivity == 26; }
DXV_HD int acc_metric(int connectivity) { return connectivity == 6 ? GEO_FACES : GEO_CHAMFER; }
DXV_HD bool acc_valid(uint32_t N, int of, int connectivity, uint32_t cap)
{
    return N >= 2u && N <= kAccMaxN && !(N & 1u) && (of == THICK_SOLID || of == THICK_EMPTY) && acc_connectivity(connectivity) && cap >= kThickMinCapSq && cap <= kThickMaxCapSq;
}

// the map's first word of a voxel of radius R (0: no member)
DXV_HD uint32_t acc_start(uint32_t R, bool seed) { return seed ? R : 0u; }

// One voxel of a tile: T is the flat array, `at` the voxel's place in it (1 .. 8 along every axis), cur = T[at], R the voxel's radius.  What the
// voxel's word becomes: the greatest of cur and what the best neighbour lets through.
template <int kConnectivity, class Tile> DXV_HD uint32_t acc_relax(const Tile* T, uint32_t at, uint32_t cur, uint32_t R)
{
    if (cur >= R) return cur;                                           // (no member, or as wide as it can get)
    uint32_t best = 0;
#pragma unroll
    for (int dz = -1; dz <= 1; ++dz)
#pragma unroll
        for (int dy = -1; dy <= 1; ++dy)
#pragma unroll
            for (int dx = -1; dx <= 1; ++dx) {
                if (!geo_weight(dx, dy, dz, acc_metric(kConnectivity))) continue;
                const uint32_t v = T[(int)at + dz * (int)kGeoPlane + dy * (int)kGeoRow + dx];
                if (v > best) best = v;
            }
    if (best > R) best = R;
    return best > cur ? best : cur;
}

// The relaxation of one tile, serially: RT holds the radii in the tile's own layout.  Swept until a sweep raises nothing, forwards and backwards
// in turn.  true: something rose.
template <int kConnectivity> inline bool acc_relax_tile(uint32_t* T, const uint32_t* RT)
{
    bool any = false;
    for (uint32_t sweep = 0; sweep < kAccMaxSweeps; ++sweep) {
        bool rose = false;
        for (uint32_t i = 0; i < kGeoTileVoxels; ++i) {
            const uint32_t k = (sweep & 1u) ? kGeoTileVoxels - 1u - i : i;
            const uint32_t at = geo_tile_at(k % kGeoTile, k / kGeoTile % kGeoTile, k / (kGeoTile * kGeoTile)), v = acc_relax<kConnectivity>(T, at, T[at], RT[at]);
            if (v != T[at]) { T[at] = v; rose = true; }
        }
        if (!rose) break;
        any = true;
    }
    return any;
}

// A voxel at (x, y, z) of its tile rose: the neighbour tiles that hold a neighbour of it under the connectivity, as bits by geo_slot
DXV_HD uint32_t acc_touch(uint32_t x, uint32_t y, uint32_t z, int connectivity) { return geo_touch(x, y, z, acc_metric(connectivity)); }

// the radius field of the paint: A in thick_radius's encoding, + for the empty kind, - for the solid one; 0 reads "no member"
DXV_HD int32_t acc_radius_word(uint32_t A, int of) { return of == THICK_EMPTY ? (int32_t)A : -(int32_t)A; }

// The tally: members reached and unreached, and the greatest word with the smallest index that holds it as one key -- the word above, the
// index's complement below.  Sums and a maximum of integers: the order of the combines does not matter.  The seeds used are counted where the
// start words are written, every member seed once (a list's duplicates: by whoever raises the word from 0), and ride along.
struct AccTally { unsigned long long seeds, reached, unreached, key; };
DXV_HD void acc_tally_voxel(AccTally& t, uint32_t word, uint32_t R, uint32_t index)
{
    if (!R) return;
    if (!word) { ++t.unreached; return; }
    ++t.reached;
    const unsigned long long key = (unsigned long long)word << 32 | (0xFFFFFFFFu - index);
    if (key > t.key) t.key = key;
}
DXV_HD void acc_tally_combine(AccTally& a, const AccTally& b)
{
    a.seeds += b.seeds; a.reached += b.reached; a.unreached += b.unreached;
    if (b.key > a.key) a.key = b.key;
}
// nothing reached: key 0 reads widest 0 at voxel 0xFFFFFFFF
DXV_HD uint32_t acc_tally_widest(const AccTally& t) { return (uint32_t)(t.key >> 32); }
DXV_HD uint32_t acc_tally_widest_voxel(const AccTally& t) { return 0xFFFFFFFFu - (uint32_t)(t.key & 0xFFFFFFFFu); }

// ---- scratch of one call: a control block, live flags and a queue of the geodesic's shape with the word the seeds are counted in between them
// (clearBytes: that word and both sets of flags, cleared together), and behind them the radius field F with the scratch of its passes -- with
// `intrusion` the whole of a thickness's scratch, which begins with F.  thick: N, F and passes always; the rest with `intrusion`. ----
struct AccScratch { GeoControl* ctl; unsigned long long* seedsUsed; uint8_t* flags[2]; size_t clearBytes; uint32_t* queue; ThickParams thick; };
inline void access_carve(Carve& c, uint32_t N, bool intrusion, AccScratch& l)
{
    l.ctl = c.take<GeoControl>(1);
    const size_t from = c.used();
    l.seedsUsed = reinterpret_cast<unsigned long long*>(c.take_bytes(256u));
    l.flags[0] = c.take<uint8_t>(geo_tiles(N));
    l.flags[1] = c.take<uint8_t>(geo_tiles(N));
    l.clearBytes = c.used() - from;
    l.queue = c.take<uint32_t>(geo_tiles(N));
    if (intrusion) { thickness_carve(c, N, l.thick); return; }
    l.thick.N = N;
    l.thick.F = c.take<int32_t>((size_t)N * N * N);
    l.thick.passes = c.take_bytes(distance_scratch_bytes(N));
}
inline size_t access_scratch_bytes(uint32_t N, bool intrusion) { return carved_bytes<AccScratch>(access_carve, N, intrusion); }

} // namespace dxv
