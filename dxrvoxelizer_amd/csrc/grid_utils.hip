// grid_utils.hip -- small streaming kernels over a finished grid or buffer: checksum, solid-voxel count, bit-packed copy.
#include "dxv_device.h"
#include "dxv_solid.h"

namespace dxv {

// Wrapping 64-bit sum of the 8-byte words of a device buffer (dxv_scene_checksum: what arrived after a broadcast is what was sent)
__global__ __launch_bounds__(256) void k_checksum(const unsigned long long* __restrict__ words, size_t n, unsigned long long* out)
{
    unsigned long long c = 0;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) c += words[i];
    for (int off = 32; off; off >>= 1) c += __shfl_down(c, off);
    if ((threadIdx.x & 63) == 0) atomicAdd(out, c);
}
hipError_t launch_checksum(const void* buf, size_t bytes, unsigned long long* out, hipStream_t s)
{
    hipError_t e = hipMemsetAsync(out, 0, sizeof(unsigned long long), s);
    if (e != hipSuccess) return e;
    const size_t n = bytes / 8;
    size_t blocks = (n + 255) / 256;
    if (blocks > 2048) blocks = 2048;
    if (blocks) k_checksum<<<(uint32_t)blocks, 256, 0, s>>>(static_cast<const unsigned long long*>(buf), n, out);
    return hipGetLastError();
}

// Solid-voxel count (a voxel is solid iff its byte is non-zero: dxv_solid.h): 16 B per lane streaming reduction, one atomic per workgroup.
__global__ __launch_bounds__(256) void k_count(const uint8_t* __restrict__ grid, size_t n, unsigned long long* out)
{
    __shared__ unsigned long long part[4];
    const size_t n16 = n / 16;
    const uint4* g16 = reinterpret_cast<const uint4*>(grid);
    unsigned long long c = 0;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n16; i += (size_t)gridDim.x * 256) {
        const uint4 v = g16[i];
        const unsigned long long lo = ((unsigned long long)v.y << 32) | v.x, hi = ((unsigned long long)v.w << 32) | v.z;
        c += solid_popc(solid_marks(lo)) + solid_popc(solid_marks(hi));     // any byte: one mark per non-zero byte
    }
    if (blockIdx.x == 0 && threadIdx.x < (n & 15)) c += solid(grid[n16 * 16 + threadIdx.x]) ? 1u : 0u;
    for (int off = 32; off; off >>= 1) c += __shfl_down(c, off);
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = c;
    __syncthreads();
    if (threadIdx.x == 0) atomicAdd(out, part[0] + part[1] + part[2] + part[3]);
}

hipError_t launch_count(const uint8_t* grid, size_t n, unsigned long long* out, hipStream_t s)
{
    hipError_t e = hipMemsetAsync(out, 0, sizeof(unsigned long long), s);
    if (e != hipSuccess) return e;
    size_t blocks = (n / 16 + 255) / 256;
    if (blocks > 2048) blocks = 2048;
    if (blocks == 0) blocks = 1;
    k_count<<<(uint32_t)blocks, 256, 0, s>>>(grid, n, out);
    return hipGetLastError();
}

// Bit-packed copy of the occupancy bytes for the host: output byte j holds voxels 8j .. 8j+7,
// voxel 8j+i in bit i, set iff the voxel's byte is non-zero (dxv_solid.h: the body's words and the tail's bytes by the same rule).
// One lane reads 16 grid bytes and writes 2; HBM bound (9/8 B per voxel).
__global__ __launch_bounds__(256) void k_pack_bits(const uint8_t* __restrict__ grid, size_t n, uint8_t* __restrict__ packed)
{
    const size_t n16 = n / 16;
    const uint4* g16 = reinterpret_cast<const uint4*>(grid);
    uint16_t* p16 = reinterpret_cast<uint16_t*>(packed);
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n16; i += (size_t)gridDim.x * 256) {
        const uint4 v = g16[i];
        const unsigned long long lo = ((unsigned long long)v.y << 32) | v.x, hi = ((unsigned long long)v.w << 32) | v.z;
        p16[i] = (uint16_t)(solid_bits(lo) | (solid_bits(hi) << 8));
    }
    if (blockIdx.x == 0 && threadIdx.x < 2) {                       // the last n % 16 voxels: at most two bytes
        const size_t first = n16 * 16 + (size_t)threadIdx.x * 8;
        if (first < n) packed[first / 8] = (uint8_t)solid_bits(grid + first, n - first);
    }
}

hipError_t launch_pack_bits(const uint8_t* grid, size_t n, uint8_t* packed, hipStream_t s)
{
    size_t blocks = (n / 16 + 255) / 256;
    if (blocks > 4096) blocks = 4096;
    if (blocks == 0) blocks = 1;
    k_pack_bits<<<(uint32_t)blocks, 256, 0, s>>>(grid, n, packed);
    return hipGetLastError();
}

} // namespace dxv
