// dxv_thickness.h -- the exact local thickness of a grid: with M the members (the solid voxels, or the empty ones),
//     D2(c) = the smallest |c - q|^2 to a voxel q of the grid outside M (dxv_distance's d2; none: +infinity)          for c in M
//     R(c)  = min(D2(c), cap_sq)                      the open ball { p : |p - c|^2 < R(c) } lies inside M
//     W(p)  = max { R(c) : c in M, |p - c|^2 < R(c) } for p in M, 0 elsewhere
// Integers only.  The routines of every stage are here, __host__ __device__: thickness.hip runs them on the GPU with a grid of threads and an
// atomic max, tests/hostcheck/thickness_check.cpp serially with a plain one.
//
// The stages.  F is DXV_DIST_SQ_I32 of the grid: one signed field gives R for either kind (thick_radius).
//   the capped part   E = { R == cap }, dE = the field of E, Top = E u { 0 < dE <= cap - 1 } = the union of the balls of radius^2 cap: W = cap there, and
//                     no such ball is painted voxel by voxel.  Elsewhere W starts as R(p): p lies in its own ball.
//   the Top cull      dT = the field of Top.  A centre of Top whose nearest voxel outside Top is at dT >= R has its ball inside Top: it raises nothing.
//   domination        a centre c with a 26-neighbour c' = c + e, R(c') > R(c) - 1 + |e|^2 + 2 ceil(sqrt(|e|^2 (R(c) - 1))), has its ball inside the
//                     ball of c' (triangle inequality on the closed radii sqrt(R - 1)): it raises nothing the chain's last centre does not.
//   paint             what is left, with R >= 2: one work item per (centre, z slice of its ball), the slice's bounding square walked in row
//                     order; W(p) = max(W(p), R) where |p - c|^2 < R.  A set function: the order of the items does not matter.
#pragma once
#include <math.h>
#include <stddef.h>
#include "dxv_types.h"
#include "dxv_distance.h"

namespace dxv {

enum { THICK_SOLID = 0, THICK_EMPTY = 1 };        // DXV_COMP_SOLID / DXV_COMP_EMPTY
enum { THICK_CULL_TOP = 1, THICK_CULL_NEIGHBOUR = 2 };                  // bits of option thickcull
constexpr uint32_t kThickMinCapSq = 2, kThickMaxCapSq = 4096;
constexpr uint32_t kThickMaxN = 1024;             // a voxel's linear index fits 30 bits, a block of the select has a 32-bit number
constexpr uint32_t kThickBlock = 1024;            // voxels per block of the select's scan: a block's items fit 20 bits, its centres 12

// floor(sqrt(v)), v < 2^24: the correctly rounded float root, put right if it is one off
DXV_HD uint32_t thick_isqrt(uint32_t v)
{
    uint32_t r = (uint32_t)sqrtf((float)v);
    if (r * r > v) --r;
    if ((r + 1u) * (r + 1u) <= v) ++r;
    return r;
}
DXV_HD uint32_t thick_ceil_sqrt(uint32_t v)
{
    const uint32_t r = thick_isqrt(v);
    return r * r == v ? r : r + 1u;
}
// the largest h with h^2 < R (R >= 1): how far the open ball of radius^2 R reaches along an axis
DXV_HD uint32_t thick_reach(uint32_t R) { return thick_isqrt(R - 1u); }

// R of a voxel from its signed squared distance (negative: solid; the sentinel is beyond every cap): 0 for a voxel that is no member
DXV_HD uint32_t thick_radius(int32_t d, int of, uint32_t cap)
{
    if (of == THICK_EMPTY ? d <= 0 : d >= 0) return 0u;
    const uint32_t mag = (uint32_t)(d < 0 ? -d : d);
    return mag < cap ? mag : cap;
}
// Top from E's byte and E's field (positive outside E; the sentinel where E is empty)
DXV_HD uint32_t thick_top(uint32_t e, int32_t dE, uint32_t cap) { return e || (dE > 0 && (uint32_t)dE <= cap - 1u) ? 1u : 0u; }
// the Top cull from Top's field (negative inside Top)
DXV_HD bool thick_inside_top(int32_t dT, uint32_t R) { return dT < 0 && (uint32_t)(-dT) >= R; }
// domination by the neighbour at squared offset e2 (1, 2 or 3) with radius Rn
DXV_HD bool thick_dominated_by(uint32_t R, uint32_t Rn, uint32_t e2) { return Rn > R - 1u + e2 + 2u * thick_ceil_sqrt(e2 * (R - 1u)); }
DXV_HD bool thick_dominated(const int32_t* F, uint32_t N, uint32_t x, uint32_t y, uint32_t z, int of, uint32_t cap, uint32_t R)
{
    for (int32_t dz = -1; dz <= 1; ++dz)
        for (int32_t dy = -1; dy <= 1; ++dy)
            for (int32_t dx = -1; dx <= 1; ++dx) {
                const uint32_t e2 = (uint32_t)(dx * dx + dy * dy + dz * dz);
                const uint32_t qx = x + (uint32_t)dx, qy = y + (uint32_t)dy, qz = z + (uint32_t)dz;
                if (!e2 || qx >= N || qy >= N || qz >= N) continue;
                if (thick_dominated_by(R, thick_radius(F[((size_t)qz * N + qy) * N + qx], of, cap), e2)) return true;
            }
    return false;
}
// the z slices of the ball of reach h round slice z that lie in the grid: how many, and the k-th
DXV_HD uint32_t thick_disc_first(uint32_t z, uint32_t h) { return z > h ? z - h : 0u; }
DXV_HD uint32_t thick_discs(uint32_t z, uint32_t h, uint32_t N) { return (z + h < N ? z + h : N - 1u) - thick_disc_first(z, h) + 1u; }

// Whether voxel (x, y, z) is a centre to paint, as the number of its work items (0: it is not).  dT: Top's field at the voxel (read only
// under THICK_CULL_TOP).
DXV_HD uint32_t thick_items(const int32_t* F, const int32_t* dT, uint32_t N, uint32_t x, uint32_t y, uint32_t z, int of, uint32_t cap, uint32_t cull)
{
    const size_t v = ((size_t)z * N + y) * N + x;
    const uint32_t R = thick_radius(F[v], of, cap);
    if (R < 2u || R == cap) return 0u;
    if ((cull & THICK_CULL_TOP) && thick_inside_top(dT[v], R)) return 0u;
    if ((cull & THICK_CULL_NEIGHBOUR) && thick_dominated(F, N, x, y, z, of, cap, R)) return 0u;
    return thick_discs(z, thick_reach(R), N);
}

// One work item: slice zz of the ball of radius^2 R round (x, y, z), shared by `lanes` callers of which this is `lane`.  raise(index, R) for
// every voxel of the slice inside the grid: the slice's bounding square in row order, so that neighbouring lanes stand on neighbouring x.
template <class Raise> DXV_HD void thick_paint_disc(uint32_t N, uint32_t x, uint32_t y, uint32_t z, uint32_t R, uint32_t zz, uint32_t lane, uint32_t lanes, Raise&& raise)
{
    const int32_t dz = (int32_t)zz - (int32_t)z;
    const uint32_t rem = R - (uint32_t)(dz * dz);                       // (> 0: |dz| <= thick_reach(R))
    const uint32_t h = thick_reach(rem), side = 2u * h + 1u, cells = side * side;
    const uint32_t stepRows = lanes / side, stepCols = lanes % side;
    uint32_t ry = lane / side, rx = lane % side;
    for (uint32_t t = lane; t < cells; t += lanes) {
        const int32_t dy = (int32_t)ry - (int32_t)h, dx = (int32_t)rx - (int32_t)h;
        const uint32_t px = x + (uint32_t)dx, py = y + (uint32_t)dy;
        if ((uint32_t)(dx * dx + dy * dy) < rem && px < N && py < N) raise(((size_t)zz * N + py) * N + px, R);
        ry += stepRows; rx += stepCols;
        if (rx >= side) { rx -= side; ++ry; }
    }
}

// What thickness.hip's stages work on: W = N^3 uint32 and hist = cap + 1 uint64 are the caller's, everything below them is scratch.
struct ThickParams {
    uint32_t N;
    int of;                           // DXV_COMP_SOLID / DXV_COMP_EMPTY
    uint32_t cap, cull;               // cap_sq; option thickcull
    uint32_t count;                   // 1: the paint counts what it tests and sends (option thickstages)
    uint32_t* W;
    unsigned long long* hist;
    int32_t *F, *G;                   // thickness_carve fills these and the ones below: the grid's field; E's field, then Top's
    uint32_t* B;                      // a byte per voxel: E, then Top, then the work items of the voxel as a centre
    unsigned long long* sums;         // per block of 1024 voxels {centres, items} in front of it, then the two totals and the paint's two counters
    uint8_t* passes;                  // distance_scratch_bytes(N)
    uint32_t *centres, *firstItem;    // the compacted centres (in G) and every centre's first item within its block (in the passes' scratch)
    const unsigned long long* counters;         // those four words behind the sums, for the host: {centres painted, work items, voxels tested, atomics sent},
                                                // the first two valid behind the select
};
inline uint32_t thick_blocks(uint32_t N) { return (uint32_t)(((size_t)N * N * N + kThickBlock - 1u) / kThickBlock); }
// scratch of one call: F and G (4 B per voxel each), B (1 B), the blocks' sums and the totals, the scratch of the fields' passes (6 B per voxel) --
// whose front holds the centres' first items once the last field is made; the centre list goes into G once the select has read it
inline void thickness_carve(Carve& c, uint32_t N, ThickParams& p)
{
    const size_t voxels = (size_t)N * N * N;
    p.N = N;
    p.F = c.take<int32_t>(voxels);
    p.G = c.take<int32_t>(voxels);
    p.centres = reinterpret_cast<uint32_t*>(p.G);
    p.B = reinterpret_cast<uint32_t*>(c.take<uint8_t>(voxels));
    p.sums = c.take<unsigned long long>(2u * ((size_t)thick_blocks(N) + 2u));
    p.counters = carve_at<const unsigned long long>(p.sums, 2u * (size_t)thick_blocks(N));
    p.passes = c.take_bytes(distance_scratch_bytes(N));
    p.firstItem = reinterpret_cast<uint32_t*>(p.passes);
}
inline size_t thickness_scratch_bytes(uint32_t N) { return carved_bytes<ThickParams>(thickness_carve, N); }

} // namespace dxv
