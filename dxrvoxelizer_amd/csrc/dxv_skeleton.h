// dxv_skeleton.h -- the skeleton graph of a whole N^3 grid (DESIGN.md §2 and include/dxv.h have the rule) on BITS: the members are one bit per
// voxel in the fill's mask layout (dxv_fill.h), adjacency is the components' at connectivity 26 (dxv_components.h).
//   classify   one 64-voxel mask word at a time: the nine rows around the word give 26 bit planes -- each row shifted by -1 (with the carry bit
//              of the word before it), by 0 and by +1 (with the carry bit of the word behind it), the centre row's own plane left out --; the
//              three planes of a row are carry-saved into a sum and a carry plane, and the nine 2-bit values are added into a bit-sliced
//              counter of two planes that saturates at 3.  deg == 2 is a curve voxel, every other member a node voxel; deg <= 1 an end.
//   label      the components' union-find, as it is, over the node mask and over the curve mask: the two are disjoint, so they share one
//              parent array, which is the label buffer; a root is the smallest index of its node or branch.
//   stats      per run of node voxels and per curve voxel, integer sums, minima, maxima and ORs: no arrival order shows.  A step {p, q} is
//              counted at its curve voxel, a curve-curve one at the smaller index; an attachment lowers a, raises b and adds 1 to its node.
//   tables     the 32-byte node records and the 48-byte branch records; a branch nobody attached to is a closed cycle (a = b = 0); the spur
//              flag from the nodes' finished records.
//   prune      a spur with 3 steps[0] + 4 steps[1] + 5 steps[2] <= max_len345 goes, with its tip.
// What deg == 2 gives: a branch is a simple path or a simple closed cycle of curve voxels; two adjacent curve voxels are in one branch; a path has
// exactly two attachments (a one-voxel path has both), steps = voxels + 1; a cycle has none, at least 3 voxels, steps = voxels.
// Everything here is __host__ __device__: skeleton.hip runs it on the GPU, tests/hostcheck/skeleton_check.cpp compiles the same text for the CPU.
#pragma once
#include <stddef.h>
#include "dxv_types.h"
#include "dxv_fill.h"
#include "dxv_components.h"

namespace dxv {

constexpr uint32_t kSkelMaxN = 1024;              // 1024^3 = 2^30 voxels: a number of a node or a branch fits the 31 bits beside the kind
constexpr uint32_t kSkelBranchBit = 0x80000000u;  // labels: 0 no member, k node k, kSkelBranchBit | b branch b
enum { SKEL_NODE_BORDER = 1, SKEL_NODE_END = 2, SKEL_NODE_JUNCTION = 4 };          // flags of a node
enum { SKEL_BRANCH_CLOSED = 1, SKEL_BRANCH_BORDER = 2, SKEL_BRANCH_SPUR = 4 };     // flags of a branch

// the tables' records, little endian (include/dxv.h)
struct SkelNode {
    uint32_t first, voxels, degree, flags;
    uint16_t lo[3], hi[3];
    uint32_t w_max;
};
struct SkelBranch {
    uint32_t a, b, first, voxels, steps[3], flags;
    uint32_t w_min, w_max;
    uint64_t w_sum;
};
static_assert(sizeof(SkelNode) == 32 && sizeof(SkelBranch) == 48, "the tables' records are 32 and 48 bytes");
// what the stats pass gathers per node with 32-bit integer atomics before the table is packed (a branch gathers into its own record)
struct SkelNodeStats : BoxStats { uint32_t degree, w_max; };

DXV_HD bool skel_valid(uint32_t N) { return N >= 2u && N <= kSkelMaxN && !(N & 1u); }

// ---- classify ----
// a saturating bit-sliced counter, 0 .. 3 per bit position
struct SkelCount {
    uint64_t b0 = 0, b1 = 0;
    // + s + 2 c per position
    DXV_HD void add(uint64_t s, uint64_t c)
    {
        const uint64_t carry0 = b0 & s, sum0 = b0 ^ s;
        const uint64_t sum1 = b1 ^ c ^ carry0, over = (b1 & c) | (b1 & carry0) | (c & carry0);
        b0 = sum0 | over; b1 = sum1 | over;
    }
};
// the three words of one row around word w: the word before it (its bit 63 is the carry of the shift by -1), the word, the word behind it
struct SkelRow { uint64_t prev, cur, next; };
DXV_HD void skel_add_row(SkelCount& n, const SkelRow& r, bool centre)
{
    const uint64_t L = r.cur << 1 | r.prev >> 63, R = r.cur >> 1 | r.next << 63, C = centre ? 0ull : r.cur;
    n.add(L ^ C ^ R, (L & C) | (L & R) | (C & R));
}
// rows[k], k = (dz + 1) * 3 + (dy + 1): the nine rows around the word, zeros for a row outside the grid; rows[4] is the word's own.
// node | curve = the word's members; ends: the members with deg <= 1; junctions: with deg >= 3
struct SkelClass { uint64_t node, curve, ends, junctions; };
DXV_HD SkelClass skel_classify(const SkelRow rows[9])
{
    SkelCount n;
#pragma unroll
    for (uint32_t k = 0; k < 9u; ++k) skel_add_row(n, rows[k], k == 4u);
    const uint64_t m = rows[4].cur;
    SkelClass c;
    c.curve = m & n.b1 & ~n.b0;
    c.node = m & ~c.curve;
    c.ends = m & ~n.b1;
    c.junctions = m & n.b1 & n.b0;
    return c;
}
// the rows around word w of row (iy, iz) from a mask in the fill's layout
DXV_HD SkelRow skel_load_row(const uint64_t* mask, uint32_t N, int iy, int iz, uint32_t w)
{
    SkelRow r{0, 0, 0};
    if (iy < 0 || iy >= (int)N || iz < 0 || iz >= (int)N) return r;
    const uint32_t W = fill_row_words(N);
    const uint64_t* row = mask + ((size_t)iz * N + (size_t)iy) * W;
    r.cur = row[w];
    r.prev = w ? row[w - 1u] : 0ull;
    r.next = w + 1u < W ? row[w + 1u] : 0ull;
    return r;
}
DXV_HD SkelClass skel_classify_word(const uint64_t* mask, uint32_t N, uint32_t iy, uint32_t iz, uint32_t w)
{
    SkelRow rows[9];
    for (int dz = -1; dz <= 1; ++dz)
        for (int dy = -1; dy <= 1; ++dy) rows[(dz + 1) * 3 + (dy + 1)] = skel_load_row(mask, N, (int)iy + dy, (int)iz + dz, w);
    return skel_classify(rows);
}

// ---- label: the first parent of voxel p over the two masks (dxv_components.h: the start of its run inside its own word) ----
DXV_HD uint32_t skel_init_parent(const uint64_t* node, const uint64_t* curve, uint32_t N, uint32_t p)
{
    const uint32_t a = comp_init_parent(node, N, p);
    return a != kCompNone ? a : comp_init_parent(curve, N, p);
}
// whether voxel p (a linear index) has its bit in a mask of the fill's layout
DXV_HD bool skel_bit(const uint64_t* mask, uint32_t N, uint32_t p)
{
    const uint32_t row = p / N, x = p - row * N;
    return (mask[(size_t)row * fill_row_words(N) + (x >> 6)] >> (x & 63u) & 1ull) != 0ull;
}
DXV_HD uint32_t skel_label(uint32_t number, bool branch) { return branch ? kSkelBranchBit | number : number; }

// ---- stats: the steps of the curve voxel at bit x of word w of row (iy, iz).  member, curve: the masks; visit(q, dx, dy, dz, isCurve) for every
// member neighbour q of the voxel (there are two) ----
template <class Visit> DXV_HD void skel_neighbours(const uint64_t* member, const uint64_t* curve, uint32_t N, uint32_t iy, uint32_t iz, uint32_t w, uint32_t x, Visit visit)
{
    const uint32_t W = fill_row_words(N);
    for (int dz = -1; dz <= 1; ++dz)
        for (int dy = -1; dy <= 1; ++dy) {
            const int ny = (int)iy + dy, nz = (int)iz + dz;
            if (ny < 0 || ny >= (int)N || nz < 0 || nz >= (int)N) continue;
            const size_t row = (size_t)nz * N + (size_t)ny;
            for (int dx = -1; dx <= 1; ++dx) {
                if (!dx && !dy && !dz) continue;
                const int nx = (int)(64u * w + x) + dx;
                if (nx < 0 || nx >= (int)N) continue;
                const size_t at = row * W + ((uint32_t)nx >> 6);
                const uint64_t bit = 1ull << ((uint32_t)nx & 63u);
                if (!(member[at] & bit)) continue;
                visit((uint32_t)(row * N) + (uint32_t)nx, dx, dy, dz, (curve[at] & bit) != 0ull);
            }
        }
}
DXV_HD uint32_t skel_step_type(int dx, int dy, int dz) { return (uint32_t)((dx ? 1 : 0) + (dy ? 1 : 0) + (dz ? 1 : 0) - 1); }

// ---- tables ----
DXV_HD SkelNode skel_node_record(uint32_t first, const SkelNodeStats& s)
{
    SkelNode r;
    r.first = first; r.voxels = s.voxels; r.degree = s.degree; r.flags = s.flags; r.w_max = s.w_max;
    for (int a = 0; a < 3; ++a) { r.lo[a] = (uint16_t)s.lo[a]; r.hi[a] = (uint16_t)s.hi[a]; }
    return r;
}
DXV_HD bool skel_tip(const SkelNode& n) { return n.voxels == 1u && n.degree == 1u; }
// a branch's record as the stats left it (a = kCompNone and b = 0: nobody attached) -> as the table holds it.  nodes: the finished node records
DXV_HD void skel_finish_branch(SkelBranch& r, const SkelNode* nodes, bool weights)
{
    if (r.a == kCompNone) { r.a = 0u; r.b = 0u; r.flags |= SKEL_BRANCH_CLOSED; }
    else if (skel_tip(nodes[r.a - 1u]) != skel_tip(nodes[r.b - 1u])) r.flags |= SKEL_BRANCH_SPUR;
    if (!weights) { r.w_min = 0u; r.w_max = 0u; r.w_sum = 0ull; }
}

// ---- prune ----
DXV_HD uint64_t skel_len345(const SkelBranch& r) { return 3ull * r.steps[0] + 4ull * r.steps[1] + 5ull * r.steps[2]; }
DXV_HD bool skel_pruned(const SkelBranch& r, uint32_t maxLen345) { return (r.flags & SKEL_BRANCH_SPUR) && skel_len345(r) <= maxLen345; }
// the tip of a spur (exactly one of a, b is one)
DXV_HD uint32_t skel_spur_tip(const SkelBranch& r, const SkelNode* nodes) { return skel_tip(nodes[r.a - 1u]) ? r.a : r.b; }

// ---- what skeleton.hip's launches work on: labels = N^3 uint32, nodes = 32 K bytes and branches = 48 B bytes are the caller's, stats = K
// SkelNodeStats of work.  The grid is only read. ----
struct SkelParams {
    const uint8_t* grid;    // N^3 bytes, element (iz * N + iy) * N + ix; a voxel is a member iff its byte is non-zero
    uint32_t N;
    const uint32_t* weights;      // N^3 uint32 of the caller's, or nullptr
    uint32_t* labels;       // parent during the build, then the labels
    uint64_t *member, *node, *curve, *ends;     // skel_carve fills these and the five below
    uint64_t *nodeRoots, *curveRoots;
    uint32_t* counts;
    unsigned long long* sums;
    unsigned long long* totals;   // {K, B, end voxels, curve voxels, junction voxels}
    SkelNodeStats* stats;
    SkelNode* nodes;
    SkelBranch* branches;
};
// scratch of one build: the member, node, curve and end masks (a bit per voxel each; node, curve and ends one behind the other: one clear), the two
// kinds' root bits in linear order, a pair of counts per 64 voxels, the scan's block sums, {K, B, end voxels, curve voxels, junction voxels}
inline void skel_carve(Carve& c, uint32_t N, SkelParams& p)
{
    const size_t words = comp_linear_words(N);
    p.N = N;
    p.member = c.take<uint64_t>(fill_mask_words(N));
    p.node = c.take<uint64_t>(fill_mask_words(N));
    p.curve = c.take<uint64_t>(fill_mask_words(N));
    p.ends = c.take<uint64_t>(fill_mask_words(N));
    p.nodeRoots = c.take<uint64_t>(words);
    p.curveRoots = c.take<uint64_t>(words);
    p.counts = c.take<uint32_t>(2u * words);
    p.sums = c.take<unsigned long long>(2u * (size_t)scan_blocks(words));
    p.totals = c.take<unsigned long long>(5);
}
inline size_t skel_scratch_bytes(uint32_t N) { return carved_bytes<SkelParams>(skel_carve, N); }

// work of dxv_skeleton_prune: {branches removed, voxels removed}, then a flag per branch and per node; bytes: all of it, cleared by the launch
struct SkelPruneWork { unsigned long long* counters; uint8_t *goB, *goN; size_t bytes; };
inline void skel_prune_carve(Carve& c, uint32_t K, uint32_t B, SkelPruneWork& w)
{
    const size_t from = c.used();
    w.counters = c.take<unsigned long long>(2);
    w.goB = c.take<uint8_t>(B);
    w.goN = c.take<uint8_t>(K);
    w.bytes = c.used() - from;
}
inline size_t skel_prune_bytes(uint32_t K, uint32_t B) { return carved_bytes<SkelPruneWork>(skel_prune_carve, K, B); }

} // namespace dxv
