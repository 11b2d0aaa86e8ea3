// dxv_solid.h -- the library's ONE definition of a solid voxel: its byte is NON-ZERO (include/dxv.h says so for every consumer of a
// grid: dxv_grid_count, dxv_grid_download_packed, dxv_distance, dxv_mesh_distance, dxv_fill, dxv_octree, dxv_isosurface, the display
// pass).  The voxelizer and the fill write 0 / 1, but a caller may write any byte through dxv_grid_device_ptr, and 0x02, 0x80 and 0xFF
// are as solid as 0x01.  Eight voxels at a time from one 64-bit load, and the scalar form for the ragged end of a grid.
// Everything here is __host__ __device__: grid_utils.hip and fill.hip run it on the GPU, tests/test_solid_rule.py compiles the same
// text for the CPU.
#pragma once
#include <stddef.h>
#include "dxv_types.h"

namespace dxv {

DXV_HD bool solid(uint8_t voxel) { return voxel != 0; }

// eight grid bytes loaded as one word (byte k = bits 8k .. 8k+7) -> bit 8k+7 set iff byte k is non-zero, every other bit clear.
// No carry leaves a byte: 0x7f + 0x7f = 0xfe, so bit 7 of the sum says "one of the low seven bits is set" and the OR adds the byte's
// own bit 7.  The number of solid voxels among the eight is the popcount of this word.
DXV_HD uint64_t solid_marks(uint64_t eight)
{
    constexpr uint64_t k7f = 0x7f7f7f7f7f7f7f7full;
    return (((eight & k7f) + k7f) | eight) & ~k7f;
}
// ... -> the 8-bit mask "byte k is non-zero" in bit k: what one byte of a packed grid holds (voxel 8j+k in bit k of byte j).
// The product moves mark k (bit 8k+7) by 49 - 7j for j = 0 .. 7; the one with j = k lands on bit 56 + k.  8k - 7j takes every value
// once over the 64 pairs, so no two terms meet, nothing carries, and the terms below bit 56 are shifted out.
DXV_HD uint32_t solid_bits(uint64_t eight) { return (uint32_t)((solid_marks(eight) * 0x0002040810204081ull) >> 56); }
// the same mask for the ragged end of a grid: `count` bytes (1 .. 8; more are not read) one at a time, the bits behind them 0
DXV_HD uint32_t solid_bits(const uint8_t* voxels, size_t count)
{
    uint32_t b = 0;
    for (size_t k = 0; k < 8u && k < count; ++k) b |= (solid(voxels[k]) ? 1u : 0u) << k;
    return b;
}
DXV_HD uint32_t solid_popc(uint64_t marks)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return (uint32_t)__popcll(marks);
#else
    return (uint32_t)__builtin_popcountll(marks);
#endif
}

} // namespace dxv
