// dxv_partition.h -- the maximal-ball partition of a grid into regions and throats: with M the members (the solid voxels, or the
// empty ones), F the grid's DXV_DIST_SQ_I32 field and index(v) = (z N + y) N + x,
//     R(v)      = thick_radius(F[v], of, cap_sq): 0 for a voxel that is no member, min(|F|, cap_sq) for a member (dxv_thickness.h's rule)
//     u above v   iff R(u) > R(v), or R(u) == R(v) and index(u) < index(v): a strict total order on the grid's voxels
//     parent(c) = the highest voxel of the CLOSED ball { u in the grid : |u - c|^2 <= R(c) }, for c in M; a member, and c itself or above c
//     root(c)   = where the chain c, parent(c), parent(parent(c)), ... ends; one region per root, numbered 1 .. K by ascending index(root)
//     label(v)  = the number of root(v) for members, 0 elsewhere
//     a throat    per unordered pair of labels that share a face p, q = p + e, e in {+x, +y, +z}, both members, label(p) != label(q):
//                 faces = how many, neck_sq = the largest min(R(p), R(q)) among them, neck_voxel = the smallest index(p) that attains it
// Integers only; every step is a set function over the order, so any traversal gives the same bytes.  The routines of every stage are here,
// __host__ __device__: partition.hip runs them on the GPU with grids of threads and atomics, tests/hostcheck/partition_check.cpp serially.
//
// A region is a family of balls: it is 26-connected through its balls but need not be a 6-connected set.  cap_sq bounds the search's reach: a
// body thicker than the cap may fall into several regions.  A tube of constant width is cut into pieces about its diameter long.
//
// The order as ONE unsigned compare: key(v) = R(v) << 32 | (0xFFFFFFFF - index(v)), 0 for a voxel that is no member.  The parent search is the
// argmax of the keys over the ball, pruned by a max-mip of the keys over 4^3 bricks and one over 16^3 cells above it (PartSearch): a cell is
// skipped when its maximum cannot beat the best so far or when its nearest point lies outside the ball, taken wholesale when its farthest point
// lies inside, descended into otherwise.  Option partprune switches the two levels off one by one; the argmax does not depend on it.
#pragma once
#include <stddef.h>
#include "dxv_types.h"
#include "dxv_thickness.h"

namespace dxv {

enum { PART_SOLID = 0, PART_EMPTY = 1 };          // DXV_COMP_SOLID / DXV_COMP_EMPTY
enum { PART_PRUNE_4 = 1, PART_PRUNE_16 = 2 };     // bits of option partprune
constexpr uint32_t kPartMinCapSq = 1, kPartMaxCapSq = 4096;
constexpr uint32_t kPartNone = 0xFFFFFFFFu;       // the parent and the root of a voxel that is no member
constexpr uint32_t kPartBlock = 1024;             // voxels, or sorted faces, per block of a scan

// the table's record, 32 bytes, and a throat's, 20 bytes (include/dxv.h)
struct PartRegion {
    uint32_t root, radius_sq, voxels, throats;
    uint16_t lo[3], hi[3];
    uint32_t flags;                               // bit 0: a voxel of the region has a coordinate 0 or N - 1
};
struct PartThroat { uint32_t a, b, faces, neck_sq, neck_voxel; };
static_assert(sizeof(PartRegion) == 32 && sizeof(PartThroat) == 20, "record layouts");
// what the atomics of a region's voxels work on
using PartStats = BoxStats;

DXV_HD uint64_t part_key(uint32_t R, uint32_t index) { return R ? (uint64_t)R << 32 | (uint64_t)(0xFFFFFFFFu - index) : 0ull; }
DXV_HD uint32_t part_key_radius(uint64_t key) { return (uint32_t)(key >> 32); }
DXV_HD uint32_t part_key_index(uint64_t key) { return 0xFFFFFFFFu - (uint32_t)key; }
DXV_HD uint32_t part_cells(uint32_t N, uint32_t side) { return (N + side - 1u) / side; }

// the voxels x0 .. x1, y0 .. y1, z0 .. z1 (inclusive)
struct PartBox { uint32_t x0, x1, y0, y1, z0, z1; };
DXV_HD uint32_t part_min(uint32_t a, uint32_t b) { return a < b ? a : b; }
DXV_HD uint32_t part_max(uint32_t a, uint32_t b) { return a > b ? a : b; }
// the voxels of cell (bx, by, bz) of side `side` that lie in the grid
DXV_HD PartBox part_cell_box(uint32_t bx, uint32_t by, uint32_t bz, uint32_t side, uint32_t N)
{
    return PartBox{bx * side, part_min(bx * side + side - 1u, N - 1u), by * side, part_min(by * side + side - 1u, N - 1u), bz * side, part_min(bz * side + side - 1u, N - 1u)};
}
// (of two boxes that meet)
DXV_HD PartBox part_meet(const PartBox& a, const PartBox& b)
{
    return PartBox{part_max(a.x0, b.x0), part_min(a.x1, b.x1), part_max(a.y0, b.y0), part_min(a.y1, b.y1), part_max(a.z0, b.z0), part_min(a.z1, b.z1)};
}
// the squares of the smallest and the largest |u - c| over u in lo .. hi, along one axis
DXV_HD void part_span(uint32_t c, uint32_t lo, uint32_t hi, uint32_t& near2, uint32_t& far2)
{
    const uint32_t a = c > lo ? c - lo : lo - c, b = c > hi ? c - hi : hi - c;
    const uint32_t far = a > b ? a : b, near = c >= lo && c <= hi ? 0u : (a < b ? a : b);
    near2 = near * near;
    far2 = far * far;
}

// The parent search of one centre (x, y, z) with R >= 1: run() gives the highest key of its closed ball.  kCount: the measurement build, which
// also counts the mip cells and the voxels it tests.  The own cells go first so that `best` is high early.
template <bool kCount> struct PartSearch {
    const uint64_t *keys, *mip4, *mip16;
    uint32_t N, prune, x, y, z, R;
    uint64_t best;
    unsigned long long cells, voxels;

    DXV_HD void walk(const PartBox& b)
    {
        for (uint32_t zz = b.z0; zz <= b.z1; ++zz) {
            const uint32_t dz = zz > z ? zz - z : z - zz, d1 = dz * dz;
            if (d1 > R) continue;
            for (uint32_t yy = b.y0; yy <= b.y1; ++yy) {
                const uint32_t dy = yy > y ? yy - y : y - yy, d2 = d1 + dy * dy;
                if (d2 > R) continue;
                const uint64_t* row = keys + ((size_t)zz * N + yy) * N;
                for (uint32_t xx = b.x0; xx <= b.x1; ++xx) {
                    const uint32_t dx = xx > x ? xx - x : x - xx;
                    if (kCount) ++voxels;
                    if (d2 + dx * dx > R) continue;
                    const uint64_t k = row[xx];
                    if (k > best) best = k;
                }
            }
        }
    }
    // whether a cell of maximum m and voxels c is done with: it cannot win, or lies outside the ball, or lies inside it (and wins wholesale)
    DXV_HD bool settled(uint64_t m, const PartBox& c)
    {
        if (kCount) ++cells;
        if (m <= best) return true;
        uint32_t nx, fx, ny, fy, nz, fz;
        part_span(x, c.x0, c.x1, nx, fx);
        part_span(y, c.y0, c.y1, ny, fy);
        part_span(z, c.z0, c.z1, nz, fz);
        if (nx + ny + nz > R) return true;
        if (fx + fy + fz <= R) { best = m; return true; }
        return false;
    }
    DXV_HD void cell4(uint32_t bx, uint32_t by, uint32_t bz, const PartBox& reach)
    {
        const uint32_t n4 = part_cells(N, 4u);
        const PartBox c = part_cell_box(bx, by, bz, 4u, N);
        if (!settled(mip4[((size_t)bz * n4 + by) * n4 + bx], c)) walk(part_meet(c, reach));
    }
    // the part `b` of the ball's bounding box, through the 4^3 bricks that meet it
    DXV_HD void level4(const PartBox& b)
    {
        if (!(prune & PART_PRUNE_4)) { walk(b); return; }
        const uint32_t ox = x >> 2, oy = y >> 2, oz = z >> 2;
        const bool own = ox >= b.x0 >> 2 && ox <= b.x1 >> 2 && oy >= b.y0 >> 2 && oy <= b.y1 >> 2 && oz >= b.z0 >> 2 && oz <= b.z1 >> 2;
        if (own) cell4(ox, oy, oz, b);
        for (uint32_t bz = b.z0 >> 2; bz <= b.z1 >> 2; ++bz)
            for (uint32_t by = b.y0 >> 2; by <= b.y1 >> 2; ++by)
                for (uint32_t bx = b.x0 >> 2; bx <= b.x1 >> 2; ++bx)
                    if (!(own && bx == ox && by == oy && bz == oz)) cell4(bx, by, bz, b);
    }
    DXV_HD void cell16(uint32_t cx, uint32_t cy, uint32_t cz, const PartBox& reach)
    {
        const uint32_t n16 = part_cells(N, 16u);
        const PartBox c = part_cell_box(cx, cy, cz, 16u, N);
        if (!settled(mip16[((size_t)cz * n16 + cy) * n16 + cx], c)) level4(part_meet(c, reach));
    }
    DXV_HD uint64_t run()
    {
        best = keys[((size_t)z * N + y) * N + x];
        cells = voxels = 0;
        const uint32_t h = thick_isqrt(R);                              // how far the closed ball reaches along an axis
        const PartBox b{x > h ? x - h : 0u, part_min(x + h, N - 1u), y > h ? y - h : 0u, part_min(y + h, N - 1u), z > h ? z - h : 0u, part_min(z + h, N - 1u)};
        if (!(prune & PART_PRUNE_16)) { level4(b); return best; }
        const uint32_t ox = x >> 4, oy = y >> 4, oz = z >> 4;
        cell16(ox, oy, oz, b);
        for (uint32_t cz = b.z0 >> 4; cz <= b.z1 >> 4; ++cz)
            for (uint32_t cy = b.y0 >> 4; cy <= b.y1 >> 4; ++cy)
                for (uint32_t cx = b.x0 >> 4; cx <= b.x1 >> 4; ++cx)
                    if (!(cx == ox && cy == oy && cz == oz)) cell16(cx, cy, cz, b);
        return best;
    }
};

// the maximum of the keys over brick (bx, by, bz) of the 4^3 level, and over cell (cx, cy, cz) of the 16^3 level from the level below
DXV_HD uint64_t part_mip4_of(const uint64_t* keys, uint32_t N, uint32_t bx, uint32_t by, uint32_t bz)
{
    const PartBox c = part_cell_box(bx, by, bz, 4u, N);
    uint64_t m = 0;
    for (uint32_t zz = c.z0; zz <= c.z1; ++zz)
        for (uint32_t yy = c.y0; yy <= c.y1; ++yy)
            for (uint32_t xx = c.x0; xx <= c.x1; ++xx) {
                const uint64_t k = keys[((size_t)zz * N + yy) * N + xx];
                if (k > m) m = k;
            }
    return m;
}
DXV_HD uint64_t part_mip16_of(const uint64_t* mip4, uint32_t n4, uint32_t cx, uint32_t cy, uint32_t cz)
{
    const PartBox c = part_cell_box(cx, cy, cz, 4u, n4);
    uint64_t m = 0;
    for (uint32_t zz = c.z0; zz <= c.z1; ++zz)
        for (uint32_t yy = c.y0; yy <= c.y1; ++yy)
            for (uint32_t xx = c.x0; xx <= c.x1; ++xx) {
                const uint64_t k = mip4[((size_t)zz * n4 + yy) * n4 + xx];
                if (k > m) m = k;
            }
    return m;
}

// root(v) by the parents alone (v a member): every step goes strictly up the order, so the chain ends within `voxels` steps
DXV_HD uint32_t part_root(const uint32_t* parent, uint32_t v, uint32_t voxels)
{
    for (uint32_t step = 0; step < voxels; ++step) {
        const uint32_t up = parent[v];
        if (up == v || up >= voxels) break;
        v = up;
    }
    return v;
}

// The faces of voxel p = (x, y, z) towards +x, +y, +z: bit k of the result is set where face k is an interface face under `id` -- any word per
// voxel that is kPartNone (roots) or 0 (labels) off the members and tells regions apart on them; other[k] = id of the voxel behind face k
DXV_HD uint32_t part_faces(const uint32_t* id, uint32_t off, uint32_t N, uint32_t x, uint32_t y, uint32_t z, uint32_t other[3])
{
    const size_t p = ((size_t)z * N + y) * N + x;
    const uint32_t mine = id[p];
    other[0] = other[1] = other[2] = off;
    if (mine == off) return 0u;
    if (x + 1u < N) other[0] = id[p + 1u];
    if (y + 1u < N) other[1] = id[p + N];
    if (z + 1u < N) other[2] = id[p + (size_t)N * N];
    return (other[0] != off && other[0] != mine ? 1u : 0u) | (other[1] != off && other[1] != mine ? 2u : 0u) | (other[2] != off && other[2] != mine ? 4u : 0u);
}
DXV_HD uint32_t part_popc3(uint32_t bits) { return (bits & 1u) + ((bits >> 1) & 1u) + ((bits >> 2) & 1u); }
// a pair of labels as one word, smaller label on top; `shift`: the bits of K
DXV_HD uint32_t part_label_bits(uint32_t K) { uint32_t s = 1; while (s < 32u && (K >> s)) ++s; return s; }
DXV_HD uint64_t part_pair(uint32_t la, uint32_t lb, uint32_t shift) { return (uint64_t)(la < lb ? la : lb) << shift | (uint64_t)(la < lb ? lb : la); }
DXV_HD uint32_t part_pair_a(uint64_t pair, uint32_t shift) { return (uint32_t)(pair >> shift); }
DXV_HD uint32_t part_pair_b(uint64_t pair, uint32_t shift) { return (uint32_t)(pair & ((1ull << shift) - 1ull)); }
// where `pair` stands among T sorted pairs (it is one of them; T on a miss)
DXV_HD uint32_t part_find_pair(const uint64_t* pairs, uint32_t T, uint64_t pair)
{
    uint32_t lo = 0, hi = T;
    while (lo < hi) {
        const uint32_t mid = lo + (hi - lo) / 2u;
        if (pairs[mid] < pair) lo = mid + 1u; else hi = mid;
    }
    return lo < T && pairs[lo] == pair ? lo : T;
}
// a face's neck and voxel as one word whose maximum is the throat's: the largest neck, then the smallest index
DXV_HD uint64_t part_neck_word(uint32_t neck, uint32_t p) { return (uint64_t)neck << 32 | (uint64_t)(0xFFFFFFFFu - p); }

DXV_HD uint32_t part_border(uint32_t x, uint32_t y, uint32_t z, uint32_t N) { return !x || !y || !z || x == N - 1u || y == N - 1u || z == N - 1u ? 1u : 0u; }
DXV_HD PartStats part_stats_none() { return box_stats_none(); }          // (the one init of dxv_scratch.h, under the name the host check calls)
DXV_HD PartRegion part_region(uint32_t root, uint32_t radius, const PartStats& s)
{
    return PartRegion{root, radius, s.voxels, 0u, {(uint16_t)s.lo[0], (uint16_t)s.lo[1], (uint16_t)s.lo[2]}, {(uint16_t)s.hi[0], (uint16_t)s.hi[1], (uint16_t)s.hi[2]}, s.flags};
}
DXV_HD PartThroat part_throat(uint64_t pair, uint32_t shift, uint32_t faces, uint64_t neckWord)
{
    return PartThroat{part_pair_a(pair, shift), part_pair_b(pair, shift), faces, (uint32_t)(neckWord >> 32), 0xFFFFFFFFu - (uint32_t)neckWord};
}

// What partition.hip's stages work on: labels = N^3 uint32, table = 32 K bytes (and throats = 20 T bytes) are the caller's; scratch and work are
// carved below.
struct PartParams {
    uint32_t N;
    int of;                           // DXV_COMP_SOLID / DXV_COMP_EMPTY
    uint32_t cap, prune;              // cap_sq; option partprune
    uint32_t count;                   // 1: the search counts what it tests (option partstages)
    uint32_t wantThroats;             // 1: the interface faces are counted with the roots
    uint32_t K;                       // partition_work_carve fills these two and the work pointers below
    unsigned long long faces;
    uint32_t* labels;                 // the caller's, in place from PART_STAGE_REGIONS on
    PartRegion* table;
    int32_t* F;                       // partition_carve fills these: the grid's field, and in the same words ...
    uint32_t *parent, *number;        // ... every member's parent, then the roots' numbers
    uint32_t* rootOf;
    uint64_t *keys, *mip4, *mip16;
    unsigned long long *sums, *counters;          // the blocks' sums; {mip cells tested, voxels tested} of the search (option partstages)
    uint8_t* passes;                  // distance_scratch_bytes(N)
    PartStats* stats;
    uint64_t *sortA, *sortB, *sorted, *pairs;     // the sort's two buffers; which of them holds the sorted words, and the other: the unique pairs
    uint32_t* hist;
    unsigned long long* headSums;
    uint32_t* pairCount;
    const unsigned long long *totals, *pairTotal; // for the host, behind the sums and behind the head sums: {K, interface faces}, and T
};
inline uint32_t part_blocks(size_t items) { return (uint32_t)((items + kPartBlock - 1u) / kPartBlock); }
// the sums of the blocks of a scan of `items` items, two per block, with the two totals behind them
inline size_t part_sums_words(size_t items) { return 2u * ((size_t)part_blocks(items) + 1u); }

// scratch of one call: F, then parent, then the roots' numbers (4 B per voxel); rootOf (4 B); the keys (8 B); the two mip levels; the blocks'
// sums with the totals {K, interface faces} behind them; the search's two counters; the scratch of the field's passes (6 B per voxel)
inline void partition_carve(Carve& c, uint32_t N, PartParams& p)
{
    const size_t voxels = (size_t)N * N * N, n4 = part_cells(N, 4u), n16 = part_cells(N, 16u);
    p.N = N;
    p.parent = p.number = c.take<uint32_t>(voxels);
    p.F = reinterpret_cast<int32_t*>(p.parent);
    p.rootOf = c.take<uint32_t>(voxels);
    p.keys = c.take<uint64_t>(voxels);
    p.mip4 = c.take<uint64_t>(n4 * n4 * n4);
    p.mip16 = c.take<uint64_t>(n16 * n16 * n16);
    p.sums = c.take<unsigned long long>(part_sums_words(voxels));
    p.totals = carve_at<const unsigned long long>(p.sums, 2u * (size_t)part_blocks(voxels));
    p.counters = reinterpret_cast<unsigned long long*>(c.take_bytes(256u));
    p.passes = c.take_bytes(distance_scratch_bytes(N));
}
inline size_t partition_scratch_bytes(uint32_t N) { return carved_bytes<PartParams>(partition_carve, N); }

// work of one call, sized once {K, interface faces} are known: the regions' stats; for the throats the two buffers of the sort, its histogram, the
// sums of the run heads with T behind them, and a count per pair.  The unique pairs go into the buffer the sort did not end in, the pairs' 64-bit
// neck words to the front of the one it did.  Without faces nothing of the throats is allocated -- their pointers stand where they would begin and
// nothing is launched that reads them --, and an allocation is never empty.
inline void partition_work_carve(Carve& c, uint32_t K, unsigned long long faces, PartParams& p)
{
    const size_t n = (size_t)faces;
    p.K = K; p.faces = faces;
    p.stats = c.take<PartStats>(K);
    const size_t throatsAt = c.used();
    p.sortA = c.take<uint64_t>(n);
    p.sortB = c.take<uint64_t>(n);
    p.hist = c.take<uint32_t>(n ? radix_sort_hist_words((uint32_t)n) : 0u);
    p.headSums = c.take<unsigned long long>(part_sums_words(n));
    p.pairTotal = carve_at<const unsigned long long>(p.headSums, 2u * (size_t)part_blocks(n));
    p.pairCount = c.take<uint32_t>(n);
    if (!n) c.at = throatsAt;
    if (!c.used()) (void)c.take_bytes(256u);
}
inline size_t partition_work_bytes(uint32_t K, unsigned long long faces) { return carved_bytes<PartParams>(partition_work_carve, K, faces); }

} // namespace dxv
