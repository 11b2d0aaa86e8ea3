// The library's solid rule (dxrvoxelizer_amd/csrc/dxv_solid.h) compiled for the CPU: the same text k_count and k_pack_bits run, driven here
// the way the kernels drive it -- the grid's 16-byte pieces as two 64-bit words each, then the last n % 16 bytes one at a time.
#include "../../dxrvoxelizer_amd/csrc/dxv_solid.h"

#include <string.h>

using namespace dxv;

// out[i] = solid_bits(words[i]), marks[i] = solid_marks(words[i])
extern "C" void sc_words(const uint64_t* words, size_t n, uint8_t* out, uint64_t* marks)
{
    for (size_t i = 0; i < n; ++i) {
        out[i] = (uint8_t)solid_bits(words[i]);
        marks[i] = solid_marks(words[i]);
    }
}

// the scalar form alone: count bytes (what the function is given; it reads 8 at the most)
extern "C" uint32_t sc_tail_bits(const uint8_t* voxels, size_t count) { return solid_bits(voxels, count); }

// k_pack_bits and k_count over n grid bytes: packed gets ceil(n / 8) bytes; returns the count
extern "C" uint64_t sc_pack_and_count(const uint8_t* grid, size_t n, uint8_t* packed)
{
    const size_t n16 = n / 16;
    uint64_t c = 0;
    for (size_t i = 0; i < n16; ++i) {
        uint64_t lo, hi;
        memcpy(&lo, grid + 16 * i, 8);
        memcpy(&hi, grid + 16 * i + 8, 8);
        packed[2 * i] = (uint8_t)solid_bits(lo);
        packed[2 * i + 1] = (uint8_t)solid_bits(hi);
        c += solid_popc(solid_marks(lo)) + solid_popc(solid_marks(hi));
    }
    for (size_t t = 0; t < 2; ++t) {
        const size_t first = n16 * 16 + t * 8;
        if (first < n) packed[first / 8] = (uint8_t)solid_bits(grid + first, n - first);
    }
    for (size_t k = n16 * 16; k < n; ++k) c += solid(grid[k]) ? 1u : 0u;
    return c;
}
