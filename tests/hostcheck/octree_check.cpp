// The product's octree routines (dxrvoxelizer_amd/csrc/dxv_octree.h) compiled for the CPU: the same text the kernels of octree.hip run, driven
// here in the kernels' order -- the dense cell words from the bottom level up, the "has a node" bits a word of 64 cells at a time, the
// exclusive scan of the words' counts, then the nodes at their bases -- and the checked descent for every voxel.
#include "../../dxrvoxelizer_amd/csrc/dxv_octree.h"

#include <string.h>
#include <sys/mman.h>
#include <unistd.h>
#include <vector>

using namespace dxv;

// pass 1 (nodes == null): out[0] = L, out[1] = the node count, out[2 .. 2 + L] = level_first.  pass 2: fills nodes (two words each) as well.
extern "C" int oc_build(const uint8_t* grid, uint32_t N, uint64_t* out, uint32_t* nodes)
{
    if (N < 2 || N > 2048 || (N & 1u)) return 1;
    const uint32_t L = oct_levels(N);
    const size_t cells = oct_level_offset(L), words = cells >> 6;
    std::vector<uint16_t> cw(cells, 0);
    // level L - 1 from the voxels, cells in Morton order
    for (size_t m = 0; m < oct_level_cells(L - 1u); ++m) {
        uint32_t cx, cy, cz, full = 0;
        oct_unmorton((uint32_t)m, cx, cy, cz);
        for (uint32_t o = 0; o < 8u; ++o) {
            const uint32_t x = 2u * cx + (o & 1u), y = 2u * cy + (o >> 1 & 1u), z = 2u * cz + (o >> 2);
            if (x < N && y < N && z < N && grid[((size_t)z * N + y) * N + x]) full |= 1u << o;
        }
        if (oct_morton(cx, cy, cz) != m) return 2;
        cw[oct_level_offset(L - 1u) + m] = (uint16_t)oct_cell_word(0u, full);
    }
    for (uint32_t l = L - 1u; l-- > 0u;)
        for (size_t i = 0; i < oct_level_cells(l); ++i) {
            uint32_t w[8];
            for (uint32_t o = 0; o < 8u; ++o) w[o] = cw[oct_level_offset(l + 1u) + 8u * i + o];
            cw[oct_level_offset(l) + i] = (uint16_t)oct_parent_word(w);
        }
    std::vector<uint64_t> masks(words, 0);
    std::vector<uint32_t> bases(words, 0);
    for (size_t cell = 0; cell < cells; ++cell)
        if (cell == 0u || (oct_cell_real(cell) && oct_cell_state(cw[cell]) == OCT_MIXED)) masks[cell >> 6] |= 1ull << (cell & 63u);
    uint64_t total = 0;
    for (size_t word = 0; word < words; ++word) { bases[word] = (uint32_t)total; total += oct_popc(masks[word]); }
    out[0] = L; out[1] = total;
    for (uint32_t l = 0; l < L; ++l) out[2u + l] = bases[oct_level_offset(l) >> 6];
    out[2u + L] = total;
    if (!nodes) return 0;
    if (total > kOctMaxNodes) return 1;
    for (size_t cell = 0; cell < cells; ++cell)
        if (masks[cell >> 6] >> (cell & 63u) & 1ull)
            oct_node(nodes + 2u * (size_t)oct_rank(masks.data(), bases.data(), cell), masks.data(), bases.data(), cell, oct_cell_level(cell, L), cw[cell]);
    return 0;
}

// oct_lookup for every voxel of the grid of side N: 0 / 1 into grid; returns the number of voxels the descent refused (left 0)
extern "C" uint64_t oc_expand(const uint32_t* nodes, uint32_t count, uint32_t levels, uint32_t N, uint8_t* grid)
{
    uint64_t refused = 0;
    for (uint32_t z = 0; z < N; ++z)
        for (uint32_t y = 0; y < N; ++y)
            for (uint32_t x = 0; x < N; ++x) {
                const int s = oct_lookup(nodes, count, levels, x, y, z);
                grid[((size_t)z * N + y) * N + x] = s == OCT_FULL ? 1 : 0;
                refused += s == OCT_BAD ? 1u : 0u;
            }
    return refused;
}

// oct_lookup on a copy of the tree that ENDS at a page no access is allowed to: a read behind the array would end the process
extern "C" int oc_lookup_guarded(const uint32_t* nodes, uint32_t count, uint32_t levels, uint32_t x, uint32_t y, uint32_t z)
{
    const size_t page = (size_t)sysconf(_SC_PAGESIZE), bytes = (size_t)count * 8u, span = (bytes + page - 1u) / page * page;
    uint8_t* mem = static_cast<uint8_t*>(mmap(nullptr, span + page, PROT_READ | PROT_WRITE, MAP_PRIVATE | MAP_ANONYMOUS, -1, 0));
    if (mem == MAP_FAILED) return -1;
    uint8_t* copy = mem + span - bytes;
    memcpy(copy, nodes, bytes);
    int s = -1;
    if (mprotect(mem + span, page, PROT_NONE) == 0) s = oct_lookup(reinterpret_cast<const uint32_t*>(copy), count, levels, x, y, z);
    munmap(mem, span + page);
    return s;
}
