// octree.hip -- the sparse voxel octree of a whole N^3 grid (dxv_octree.h has the rule and the dense layout), as reduce -> scan -> emit,
// so that the nodes stand level by level in Morton order whatever the scheduling, and the way back, octree -> grid:
//   k_oct_reduce     one wave per 8^3-voxel brick of the cube, bricks in Morton order.  A lane takes the 8-voxel x-run (y, z) = (lane & 7,
//                    lane >> 3) of the brick -- one aligned 8-byte load where N % 8 == 0, guarded bytes otherwise, nothing outside the grid --
//                    and keeps one bit per voxel.  Four cross-lane moves give lane m the eight voxels of the 2^3 cell with Morton code m: the
//                    brick's 64 cell words of level L - 1; two ballots of their states are the 8 words of level L - 2, two more the word
//                    of level L - 3.  All go to the dense array; the ballot of "mixed" is the brick's word of "has a node" bits.  The grid is
//                    read once, by this kernel.  (L < 3: the cube is part of one brick; the cells of a level are the first of that brick's.)
//   k_oct_level      one per level above L - 3, from L - 4 up to the root: a thread per cell, eight consecutive child words -> its word.
//   k_oct_flags      the "has a node" bits of levels 0 .. L - 2 (the root always has one), a wave per 64 cells.
//   scan.hip, k_oct_level_first
//                    the exclusive scan of the words' popcounts (launch_scan_words, one count per word), then the scan value at the start of
//                    every level and the total: level_first, the L + 1 words the host reads.
//   k_oct_emit       a wave per 64 cells: a flagged cell's node goes to its word's base + the set bits below its own; word0 is the scan value
//                    at the dense position of its child 0.
//   k_oct_expand     one wave per 8^3 brick of the GRID: a wave-uniform checked descent from the root to the brick's level-(L - 3) cell, with
//                    early out for empty and full, then every lane finishes the last three levels for its x-run and stores its 8 voxels, 0
//                    or 1 each.  Every index is compared with the node count before it is followed (oct_child); a tree that cannot be
//                    followed gives empty voxels and sets the frame's status word.
// No atomics, no workgroup waits for another, no kernel here uses scratch memory or LDS.  The scratch is laid out by oct_carve (dxv_octree.h).
#include "dxv_device.h"
#include "dxv_octree.h"

namespace dxv {

// the lane's x-run of brick (bx, by, bz): bit k set iff voxel (8 bx + k, 8 by + y, 8 bz + z) lies in the grid and its byte is non-zero
__device__ __forceinline__ uint32_t oct_load_run(const uint8_t* __restrict__ grid, uint32_t N, uint32_t bx, uint32_t by, uint32_t bz, uint32_t lane)
{
    const uint32_t gx = bx * 8u, gy = by * 8u + (lane & 7u), gz = bz * 8u + (lane >> 3);
    if (gx >= N || gy >= N || gz >= N) return 0u;
    const uint8_t* row = grid + ((size_t)gz * N + gy) * N + gx;
    uint32_t bits = 0;
    if (!(N & 7u)) {                                                    // (the grid is 256-byte aligned and every row a multiple of 8 bytes)
        const uint64_t v = *reinterpret_cast<const uint64_t*>(row);
#pragma unroll
        for (uint32_t k = 0; k < 8u; ++k) bits |= ((v >> 8u * k & 0xffull) ? 1u : 0u) << k;
    } else {
#pragma unroll
        for (uint32_t k = 0; k < 8u; ++k)
            if (gx + k < N) bits |= (row[k] ? 1u : 0u) << k;
    }
    return bits;
}

__global__ __launch_bounds__(256) void k_oct_reduce(OctParams p, uint32_t bricks)
{
    const uint32_t brick = blockIdx.x * 4u + (threadIdx.x >> 6);
    if (brick >= bricks) return;                                        // (the whole wave)
    const uint32_t lane = threadIdx.x & 63u, L = p.L;
    uint32_t bx, by, bz;
    oct_unmorton(brick, bx, by, bz);
    const uint32_t bits = oct_load_run(p.grid, p.N, bx, by, bz, lane);
    // lane m: the level-(L - 1) cell with Morton code m inside the brick, its eight voxels from four rows
    const uint32_t cx = (lane & 1u) | (lane >> 2 & 2u), cy = (lane >> 1 & 1u) | (lane >> 3 & 2u), cz = (lane >> 2 & 1u) | (lane >> 4 & 2u);
    uint32_t full = 0;
#pragma unroll
    for (uint32_t d = 0; d < 4u; ++d) {                                 // d = dy | dz << 1
        const uint32_t row = __shfl(bits, (int)((2u * cy + (d & 1u)) | (2u * cz + (d >> 1)) << 3));
        full |= (row >> 2u * cx & 3u) << 2u * d;
    }
    const uint32_t wordA = oct_cell_word(0u, full);
    const int stateA = oct_cell_state(wordA);
    const uint64_t mixedA = __ballot(stateA == OCT_MIXED), fullA = __ballot(stateA == OCT_FULL);
    const uint32_t j = lane & 7u;                                       // lanes 0 .. 7: the level-(L - 2) cell with Morton code j inside the brick
    const uint32_t wordB = oct_cell_word((uint32_t)(mixedA >> 8u * j), (uint32_t)(fullA >> 8u * j));
    const int stateB = oct_cell_state(wordB);
    const uint64_t mixedB = __ballot(lane < 8u && stateB == OCT_MIXED), fullB = __ballot(lane < 8u && stateB == OCT_FULL);
    const uint32_t wordC = oct_cell_word((uint32_t)mixedB, (uint32_t)fullB);
    // a cube smaller than a brick: the cells of a level are the first 8^level of the brick's
    const uint32_t cellsA = L >= 3u ? 64u : 1u << 3u * (L - 1u), cellsB = L >= 3u ? 8u : L == 2u ? 1u : 0u;
    const size_t firstA = oct_level_offset(L - 1u) + (size_t)brick * 64u;
    if (lane < cellsA) p.cells[firstA + lane] = (uint16_t)wordA;
    if (lane < cellsB) p.cells[oct_level_offset(L - 2u) + (size_t)brick * 8u + lane] = (uint16_t)wordB;
    if (L >= 3u && lane == 0u) p.cells[oct_level_offset(L - 3u) + brick] = (uint16_t)wordC;
    const uint64_t nodes = __ballot(lane < cellsA && (L == 1u || stateA == OCT_MIXED));     // (L == 1: the one cell is the root, which always has a node)
    if (lane == 0u) { p.masks[firstA >> 6] = nodes; p.bases[firstA >> 6] = oct_popc(nodes); }
}

// level l from level l + 1: eight consecutive child words (16 aligned bytes) -> the cell's word
__global__ __launch_bounds__(256) void k_oct_level(uint16_t* __restrict__ cells, uint32_t l)
{
    const size_t i = (size_t)blockIdx.x * 256u + threadIdx.x;
    if (i >= oct_level_cells(l)) return;
    const uint4 v = *reinterpret_cast<const uint4*>(cells + oct_level_offset(l + 1u) + 8u * i);
    const uint32_t w[8] = {v.x & 0xffffu, v.x >> 16, v.y & 0xffffu, v.y >> 16, v.z & 0xffffu, v.z >> 16, v.w & 0xffffu, v.w >> 16};
    cells[oct_level_offset(l) + i] = (uint16_t)oct_parent_word(w);
}

// "has a node" for the dense words in front of level L - 1: the root, and every mixed cell (padding is never read)
__global__ __launch_bounds__(256) void k_oct_flags(OctParams p, size_t words)
{
    const size_t word = (size_t)blockIdx.x * 4u + (threadIdx.x >> 6);
    if (word >= words) return;                                          // (the whole wave)
    const uint32_t lane = threadIdx.x & 63u;
    const size_t cell = word * 64u + lane;
    const bool node = cell == 0u || (oct_cell_real(cell) && oct_cell_state(p.cells[cell]) == OCT_MIXED);
    const uint64_t nodes = __ballot(node);
    if (lane == 0u) { p.masks[word] = nodes; p.bases[word] = oct_popc(nodes); }
}

// level_first[l] = the nodes in front of level l (every level starts a word); level_first[L], the total, is in place
__global__ __launch_bounds__(64) void k_oct_level_first(OctParams p)
{
    if (threadIdx.x < p.L) p.levelFirst[threadIdx.x] = p.bases[oct_level_offset(threadIdx.x) >> 6];
}

__global__ __launch_bounds__(256) void k_oct_emit(OctParams p, size_t words)
{
    const size_t word = (size_t)blockIdx.x * 4u + (threadIdx.x >> 6);
    if (word >= words) return;
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t mask = p.masks[word];
    if (!(mask >> lane & 1ull)) return;
    const size_t cell = word * 64u + lane;
    uint32_t node[2];
    oct_node(node, p.masks, p.bases, cell, oct_cell_level(cell, p.L), p.cells[cell]);
    reinterpret_cast<uint2*>(p.nodes)[p.bases[word] + oct_popc(mask & ((1ull << lane) - 1ull))] = make_uint2(node[0], node[1]);
}

__global__ __launch_bounds__(256) void k_oct_expand(uint8_t* __restrict__ grid, uint32_t N, uint32_t L, const uint32_t* __restrict__ nodes, uint32_t count,
                                                    uint32_t* __restrict__ bad)
{
    const uint32_t side = (N + 7u) / 8u, bricks = side * side * side;
    const uint32_t brick = blockIdx.x * 4u + (threadIdx.x >> 6);
    if (brick >= bricks) return;                                        // (the whole wave)
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t bx = brick % side, by = brick / side % side, bz = brick / side / side;
    // the wave's part: from the root to the brick's cell of level L - 3 (L <= 3: that is the root, whose node always exists)
    uint32_t n = 0;
    int state = OCT_MIXED;
    for (uint32_t l = 0; l + 3u < L && state == OCT_MIXED; ++l) state = oct_child(nodes, count, n, oct_octant(bx, by, bz, L - 4u - l));
    // the lane's part: the last `rest` levels for the cells along its x-run, each as far down as it is mixed
    const uint32_t rest = L < 3u ? L : 3u, y = lane & 7u, z = lane >> 3;
    uint32_t run = state == OCT_FULL ? 0xffu : 0u;
    bool refused = state == OCT_BAD;
    if (state == OCT_MIXED) {
        for (uint32_t x = 0; x < (1u << rest);) {
            uint32_t m = n, k = 0;
            int s = OCT_MIXED;
            while (k < rest && s == OCT_MIXED) { s = oct_child(nodes, count, m, oct_octant(x, y, z, rest - 1u - k)); ++k; }
            const uint32_t span = 1u << (rest - k);                     // the side of the cell the descent ended in: x is its first voxel
            if (s == OCT_FULL) run |= ((1u << span) - 1u) << x;
            refused |= s == OCT_BAD || s == OCT_MIXED;                  // (still mixed after L levels: a voxel is not)
            x += span;
        }
    }
    if (refused) bad[0] = 1u;
    const uint32_t gx = bx * 8u, gy = by * 8u + y, gz = bz * 8u + z;
    if (gy >= N || gz >= N) return;
    uint8_t* row = grid + ((size_t)gz * N + gy) * N + gx;
    if (!(N & 7u)) {
        uint64_t v = 0;
#pragma unroll
        for (uint32_t k = 0; k < 8u; ++k) v |= (uint64_t)(run >> k & 1u) << 8u * k;
        *reinterpret_cast<uint64_t*>(row) = v;
    } else {
#pragma unroll
        for (uint32_t k = 0; k < 8u; ++k)
            if (gx + k < N) row[k] = (uint8_t)(run >> k & 1u);
    }
}

static bool oct_params_ok(const OctParams& p) { return p.N >= 2u && p.N <= 2048u && !(p.N & 1u) && p.L == oct_levels(p.N) && p.grid && p.cells; }

// reduce + scan: the dense cell words, p.masks and p.bases (the nodes in front of every word) and p.levelFirst[0 .. L]
hipError_t launch_oct_count(const OctParams& p, hipStream_t s)
{
    if (!oct_params_ok(p)) return hipErrorInvalidValue;
    const uint32_t L = p.L, bricks = L > 3u ? 1u << 3u * (L - 3u) : 1u;
    const size_t words = oct_words(L), upper = oct_level_offset(L - 1u) >> 6;
    k_oct_reduce<<<(bricks + 3u) / 4u, 256, 0, s>>>(p, bricks);
    for (uint32_t l = L; l-- > 3u;) {                                   // levels L - 4 .. 0
        const uint32_t level = l - 3u;
        k_oct_level<<<(uint32_t)((oct_level_cells(level) + 255u) / 256u), 256, 0, s>>>(p.cells, level);
    }
    if (upper) k_oct_flags<<<(uint32_t)((upper + 3u) / 4u), 256, 0, s>>>(p, upper);
    const hipError_t e = launch_scan_words(p.bases, 1, words, p.sums, p.levelFirst + L, s);
    if (e != hipSuccess) return e;
    k_oct_level_first<<<1, 64, 0, s>>>(p);
    return hipGetLastError();
}

// emit: p.nodes (levelFirst[L] nodes of 8 bytes) from what launch_oct_count left
hipError_t launch_oct_emit(const OctParams& p, hipStream_t s)
{
    if (!oct_params_ok(p) || !p.nodes) return hipErrorInvalidValue;
    const size_t words = oct_words(p.L);
    k_oct_emit<<<(uint32_t)((words + 3u) / 4u), 256, 0, s>>>(p, words);
    return hipGetLastError();
}

// the grid of side N from a tree of `count` nodes of oct_levels(N) levels, 4-byte aligned; *bad is set to 1 if the tree cannot be followed
hipError_t launch_oct_expand(uint8_t* grid, uint32_t N, const uint32_t* nodes, uint32_t count, uint32_t* bad, hipStream_t s)
{
    if (N < 2u || N > 2048u || (N & 1u) || !grid || !nodes || !count || !bad) return hipErrorInvalidValue;
    const uint32_t side = (N + 7u) / 8u, bricks = side * side * side;
    k_oct_expand<<<(bricks + 3u) / 4u, 256, 0, s>>>(grid, N, oct_levels(N), nodes, count, bad);
    return hipGetLastError();
}

} // namespace dxv
