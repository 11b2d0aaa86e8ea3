// dxv_octree.h -- the sparse voxel octree of a whole N^3 grid (DESIGN.md §2 has the rule).  The cube [0, S)^3, S the smallest power of two
// >= N and L = log2 S, is cut into cells: a cell of level l has side S >> l, a level-L cell is a voxel (full iff its byte is non-zero;
// voxels of the cube outside the grid are empty), a cell above is empty / full when its eight children all are, else mixed.  One 8-byte
// node for the root and for every mixed cell of levels 1 .. L - 1, levels one after another, ascending Morton code inside a level:
//     word1 = mixed | full << 8   (bit o = dx | dy << 1 | dz << 2 of each: child o is mixed / full)  -- the CELL WORD of the node's cell
//     word0 = the node of the lowest-numbered mixed child (0 when there is none); mixed child o: word0 + popcount(mixed & ((1 << o) - 1))
// The build keeps the cell words of ALL cells of levels 0 .. L - 1 in one dense array -- level l at oct_level_offset(l), Morton order inside
// it, levels 0 and 1 padded to 64 cells so that every level starts a 64-cell word --, one bit per cell for "has a node", and the exclusive
// scan of the words' popcounts: a node's number is its word's base + the set bits below its own, whatever the scheduling.
// Everything here is __host__ __device__: octree.hip runs it on the GPU, tests/test_octree_rule.py compiles the same text for the CPU.
#pragma once
#include <stddef.h>
#include "dxv_types.h"
#include "dxv_scratch.h"

namespace dxv {

constexpr uint32_t kOctMaxLevels = 11;                                  // S <= 2048
constexpr uint64_t kOctMaxNodes = 0x7fffffffull;                        // nodes of a tree at the most

enum { OCT_EMPTY = 0, OCT_FULL = 1, OCT_MIXED = 2, OCT_BAD = 3 };       // a cell's state; OCT_BAD: a tree that cannot be followed (oct_child)

DXV_HD uint32_t oct_popc(uint64_t v)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return (uint32_t)__popcll(v);
#else
    return (uint32_t)__builtin_popcountll(v);
#endif
}

// L of a grid of side N (2 <= N <= 2048): the smallest L with (1 << L) >= N
DXV_HD uint32_t oct_levels(uint32_t N)
{
    uint32_t L = 1;
    while ((1u << L) < N) ++L;
    return L;
}

// Morton code of a cell position: per bit triple x is the lowest bit, then y, then z (11 bits per axis at the most)
DXV_HD uint32_t oct_spread(uint32_t v)
{
    v &= 0x7ffu;
    v = (v | v << 16) & 0x070000ffu;
    v = (v | v << 8) & 0x0700f00fu;
    v = (v | v << 4) & 0x430c30c3u;
    v = (v | v << 2) & 0x49249249u;
    return v;
}
DXV_HD uint32_t oct_compact(uint32_t v)
{
    v &= 0x49249249u;
    v = (v | v >> 2) & 0x430c30c3u;
    v = (v | v >> 4) & 0x0700f00fu;
    v = (v | v >> 8) & 0x070000ffu;
    v = (v | v >> 16) & 0x7ffu;
    return v;
}
// (positions of up to 10 bits per axis: the cells of levels 0 .. L - 1, and the 8^3 bricks of the cube)
DXV_HD uint32_t oct_morton(uint32_t x, uint32_t y, uint32_t z) { return oct_spread(x) | oct_spread(y) << 1 | oct_spread(z) << 2; }
DXV_HD void oct_unmorton(uint32_t m, uint32_t& x, uint32_t& y, uint32_t& z) { x = oct_compact(m); y = oct_compact(m >> 1); z = oct_compact(m >> 2); }

// the node word1 / cell word of a cell from its children's bits, and what it says about the cell itself
DXV_HD uint32_t oct_cell_word(uint32_t mixed, uint32_t full) { return (mixed & 0xffu) | (full & 0xffu) << 8; }
DXV_HD uint32_t oct_word_mixed(uint32_t word) { return word & 0xffu; }
DXV_HD uint32_t oct_word_full(uint32_t word) { return word >> 8 & 0xffu; }
DXV_HD int oct_cell_state(uint32_t word) { return word == 0u ? OCT_EMPTY : word == 0xff00u ? OCT_FULL : OCT_MIXED; }
// a cell word from the words of its eight children, child o in w[o]
DXV_HD uint32_t oct_parent_word(const uint32_t w[8])
{
    uint32_t mixed = 0, full = 0;
    for (uint32_t o = 0; o < 8u; ++o) {
        const int s = oct_cell_state(w[o]);
        mixed |= (s == OCT_MIXED ? 1u : 0u) << o;
        full |= (s == OCT_FULL ? 1u : 0u) << o;
    }
    return oct_cell_word(mixed, full);
}

// the dense array of cell words: where level l starts (levels 0 and 1 take 64 cells each), so oct_level_offset(L) cells in all
DXV_HD size_t oct_level_offset(uint32_t l) { return l < 2u ? 64u * (size_t)l : 128u + (((size_t)1 << 3u * l) - 64u) / 7u; }
DXV_HD size_t oct_level_cells(uint32_t l) { return (size_t)1 << 3u * l; }
// the level of dense cell `cell` of a tree of L levels (a padding cell counts to the level in front of it)
DXV_HD uint32_t oct_cell_level(size_t cell, uint32_t L)
{
    uint32_t l = 0;
    while (l + 1u < L && cell >= oct_level_offset(l + 1u)) ++l;
    return l;
}
// whether dense cell `cell` is a cell at all, not padding
DXV_HD bool oct_cell_real(size_t cell) { return cell >= 128u || cell == 0u || (cell >= 64u && cell < 72u); }

// the scan value at dense position `cell`: the nodes in front of it
DXV_HD uint32_t oct_rank(const uint64_t* masks, const uint32_t* bases, size_t cell)
{
    return bases[cell >> 6] + oct_popc(masks[cell >> 6] & ((1ull << (cell & 63u)) - 1ull));
}
// the node of flagged dense cell `cell` (level l, cell word `word`): word0 = the scan value at the dense position of its child 0
DXV_HD void oct_node(uint32_t out[2], const uint64_t* masks, const uint32_t* bases, size_t cell, uint32_t l, uint32_t word)
{
    out[1] = word;
    out[0] = oct_word_mixed(word) ? oct_rank(masks, bases, oct_level_offset(l + 1u) + 8u * (cell - oct_level_offset(l))) : 0u;
}

// One step of a descent: child o of node n (n < count).  OCT_FULL / OCT_EMPTY: the child is that, n is left alone.  OCT_MIXED: n becomes the
// child's node, which lies inside the array but has not been read.  OCT_BAD: the index the node gives lies outside the array; nothing is read
// there.  (A child flagged both full and mixed counts as full.)
DXV_HD int oct_child(const uint32_t* nodes, uint32_t count, uint32_t& n, uint32_t o)
{
    const uint32_t word = nodes[2u * (size_t)n + 1u];
    if (oct_word_full(word) >> o & 1u) return OCT_FULL;
    const uint32_t mixed = oct_word_mixed(word);
    if (!(mixed >> o & 1u)) return OCT_EMPTY;
    const uint64_t child = (uint64_t)nodes[2u * (size_t)n] + oct_popc(mixed & ((1u << o) - 1u));
    if (child >= count) return OCT_BAD;
    n = (uint32_t)child;
    return OCT_MIXED;
}
// the octant of position (x, y, z) -- of a voxel, or of anything measured in units of `1 << shift` voxels -- at the level whose children
// have that side
DXV_HD uint32_t oct_octant(uint32_t x, uint32_t y, uint32_t z, uint32_t shift) { return (x >> shift & 1u) | (y >> shift & 1u) << 1 | (z >> shift & 1u) << 2; }

// The checked descent: voxel (x, y, z) of the cube of a tree of `count` >= 1 nodes and `levels` levels -> OCT_EMPTY / OCT_FULL, or OCT_BAD
// for a tree that cannot be followed: an index at or beyond `count`, or a cell that is still mixed after `levels` steps (a voxel is not;
// a node that points at itself ends here).  Every index is compared with `count` before it is followed: no read outside the array.
DXV_HD int oct_lookup(const uint32_t* nodes, uint32_t count, uint32_t levels, uint32_t x, uint32_t y, uint32_t z)
{
    uint32_t n = 0;
    for (uint32_t l = 0; l < levels; ++l) {
        const int s = oct_child(nodes, count, n, oct_octant(x, y, z, levels - 1u - l));
        if (s != OCT_MIXED) return s;
    }
    return OCT_BAD;
}

// ---- what octree.hip's launches work on: nodes (8 bytes each) is the caller's ----
struct OctParams {
    const uint8_t* grid;    // N^3 bytes, element (iz * N + iy) * N + ix; a voxel is solid iff its byte is non-zero
    uint32_t N, L;          // oct_carve fills L and the five below
    uint16_t* cells;        // the dense cell words
    uint64_t* masks;        // "has a node", one bit per dense cell
    uint32_t* bases;        // per 64 cells: the nodes among them, then the nodes in front of them
    unsigned long long* sums;
    unsigned long long* levelFirst;   // [0 .. L]: the nodes in front of every level, and the total
    uint32_t* nodes;
};
inline size_t oct_words(uint32_t L) { return oct_level_offset(L) >> 6; }
// scratch of one build: the dense cell words (2 bytes per cell of levels 0 .. L - 1), their "has a node" bits, the words' counts / bases, the
// scan's block sums, level_first
inline void oct_carve(Carve& c, uint32_t N, OctParams& p)
{
    const uint32_t L = oct_levels(N);
    const size_t words = oct_words(L);
    p.N = N; p.L = L;
    p.cells = c.take<uint16_t>(words * 64u);
    p.masks = c.take<uint64_t>(words);
    p.bases = c.take<uint32_t>(words);
    p.sums = c.take<unsigned long long>(scan_blocks(words));
    p.levelFirst = c.take<unsigned long long>(kOctMaxLevels + 1u);
}
inline size_t oct_scratch_bytes(uint32_t N) { return carved_bytes<OctParams>(oct_carve, N); }

} // namespace dxv
