// dxv_scan.h -- the exclusive scan over a workgroup, the one device routine under every prefix sum of the grid operators: scan.hip's three
// kernels (octree, components, isosurface; the block sums of thickness and partition) and the scans inside a block of 1024 voxels that
// thickness.hip and partition.hip make in their own kernels.  Integer addition only: the result does not depend on the order of the adds.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace dxv {

// two sums that are scanned side by side (isosurface: vertices and quads; thickness: centres and items; partition: roots and faces)
struct ScanPair { unsigned long long a, b; };
__device__ __forceinline__ ScanPair operator+(ScanPair x, ScanPair y) { return ScanPair{x.a + y.a, x.b + y.b}; }
__device__ __forceinline__ ScanPair operator-(ScanPair x, ScanPair y) { return ScanPair{x.a - y.a, x.b - y.b}; }

__device__ __forceinline__ uint32_t scan_shfl_up(uint32_t v, uint32_t d) { return (uint32_t)__shfl_up((int)v, d); }
__device__ __forceinline__ unsigned long long scan_shfl_up(unsigned long long v, uint32_t d) { return __shfl_up(v, d); }
__device__ __forceinline__ ScanPair scan_shfl_up(ScanPair v, uint32_t d) { return ScanPair{__shfl_up(v.a, d), __shfl_up(v.b, d)}; }

// exclusive scan of one value per thread over a workgroup of kWaves whole waves (T: uint32_t, unsigned long long or ScanPair); total: the
// workgroup's sum, in every thread.  Every thread of the workgroup calls it; kWaves * sizeof(T) bytes of LDS.
template <class T, uint32_t kWaves> __device__ __forceinline__ T block_scan_exclusive(T mine, T& total)
{
    __shared__ T waveSums[kWaves];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    T inc = mine;
#pragma unroll
    for (uint32_t d = 1; d < 64u; d <<= 1) {
        const T v = scan_shfl_up(inc, d);
        if (lane >= d) inc = inc + v;
    }
    if (lane == 63u) waveSums[wave] = inc;
    __syncthreads();
    T before{};
    total = T{};
    for (uint32_t k = 0; k < kWaves; ++k) {
        if (k < wave) before = before + waveSums[k];
        total = total + waveSums[k];
    }
    __syncthreads();                                                    // (the sums may be written again by the caller's next scan)
    return before + inc - mine;
}

} // namespace dxv
