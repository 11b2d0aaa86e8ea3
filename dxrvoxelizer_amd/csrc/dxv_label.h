// dxv_label.h -- what components.hip and skeleton.hip share behind the union-find: the device side of
//   numbering   the roots of a compressed parent array -- parent[p] == p -- as bits in LINEAR order, for C kinds of root with C interleaved
//               counts per 64 voxels (scan.hip's launch_scan_words turns them into the roots in front of every word, per kind); C = 1: the
//               components; C = 2: the skeleton, where a root whose voxel is in a second mask (the curve mask) is of the second kind, its label
//               carries kSkelBranchBit, and its `first` goes into the second table
//   stats       stat_add / stat_min / stat_max / stat_or, relaxed agent-scope atomics sent only where they change what a relaxed load shows;
//               BoxRun, what one run of voxels along x adds to its BoxStats (dxv_scratch.h): one init, one reduction over a wave, one send
//   edit        the pass over labels and grid that clears or sets the bytes of the voxels whose label a predicate names
// The kernels are templates: each translation unit instantiates its own (components.hip C = 1, skeleton.hip C = 2).  None uses scratch memory
// or LDS, none waits for another workgroup, every loop is bounded by the bits of a word.
#pragma once
#include <hip/hip_runtime.h>
#include "dxv_skeleton.h"

namespace dxv {

// In all of them bits0 / bits1 are the root bits of the first and of the second kind (bits1 unused for C = 1), counts the C interleaved counts per
// 64 voxels -- behind the scan: the roots of each kind in front of the word.

// a wave per 64 voxels in linear order; C = 2: `second` is the mask (the fill's layout, side N) of the voxels whose root is of the second kind
template <uint32_t C> __global__ __launch_bounds__(256) void k_label_roots(const uint32_t* __restrict__ parent, const uint64_t* __restrict__ second, uint32_t N, uint32_t total,
                                                                          uint64_t* __restrict__ bits0, uint64_t* __restrict__ bits1, uint32_t* __restrict__ counts, uint32_t words)
{
    const uint32_t word = blockIdx.x * 4u + (threadIdx.x >> 6);
    if (word >= words) return;                                          // (the whole wave)
    const uint32_t lane = threadIdx.x & 63u;
    const size_t p = (size_t)word * 64u + lane;
    const bool root = p < total && parent[p] == (uint32_t)p;
    if constexpr (C == 1) {
        const uint64_t roots = __ballot(root);
        if (lane == 0u) { bits0[word] = roots; counts[word] = comp_popc(roots); }
    } else {
        const bool ofSecond = root && skel_bit(second, N, (uint32_t)p);
        const uint64_t r0 = __ballot(root && !ofSecond), r1 = __ballot(ofSecond);
        if (lane == 0u) {
            bits0[word] = r0; bits1[word] = r1;
            counts[2u * word] = comp_popc(r0); counts[2u * word + 1u] = comp_popc(r1);
        }
    }
}

// the label of a voxel whose root is `root`: the rank of the root among its kind's roots + 1, with kSkelBranchBit for the second kind
template <uint32_t C> __device__ __forceinline__ uint32_t label_of(uint32_t root, const uint64_t* __restrict__ bits0, const uint64_t* __restrict__ bits1, const uint32_t* __restrict__ counts)
{
    if (root == kCompNone) return 0u;
    const uint32_t word = root >> 6;
    const uint64_t below = (1ull << (root & 63u)) - 1ull;
    if constexpr (C == 1) return counts[word] + comp_popc(bits0[word] & below) + 1u;
    else {
        const uint64_t r1 = bits1[word];
        const bool ofSecond = (r1 >> (root & 63u) & 1ull) != 0ull;
        const uint32_t rank = ofSecond ? counts[2u * word + 1u] + comp_popc(r1 & below) : counts[2u * word] + comp_popc(bits0[word] & below);
        return skel_label(rank + 1u, ofSecond);
    }
}
// four consecutive voxels per thread, in place (a lane reads only its own entries of the buffer it writes)
template <uint32_t C> __global__ __launch_bounds__(256) void k_label_number(uint32_t* labels, uint32_t total, const uint64_t* __restrict__ bits0, const uint64_t* __restrict__ bits1,
                                                                           const uint32_t* __restrict__ counts)
{
    const size_t first = ((size_t)blockIdx.x * 256u + threadIdx.x) * 4u;
    if (first >= total) return;
    uint4* at = reinterpret_cast<uint4*>(labels + first);
    const uint4 r = *at;
    *at = make_uint4(label_of<C>(r.x, bits0, bits1, counts), label_of<C>(r.y, bits0, bits1, counts), label_of<C>(r.z, bits0, bits1, counts), label_of<C>(r.w, bits0, bits1, counts));
}

// one lane per 64 voxels in linear order: the roots among them are the `first` of consecutive records of their kind's table (n0, n1 records;
// C = 1: no second table)
template <uint32_t C, class R0, class R1> __global__ __launch_bounds__(256) void k_label_first(const uint64_t* __restrict__ bits0, const uint64_t* __restrict__ bits1,
                                                                                              const uint32_t* __restrict__ counts, uint32_t words, R0* __restrict__ table0, uint32_t n0,
                                                                                              R1* __restrict__ table1, uint32_t n1)
{
    const uint32_t word = blockIdx.x * 256u + threadIdx.x;
    if (word >= words) return;
    uint64_t roots = bits0[word];
    for (uint32_t k = counts[C * word]; roots && k < n0; ++k) {
        table0[k].first = word * 64u + comp_ctz(roots);
        roots &= roots - 1ull;
    }
    if constexpr (C == 2) {
        roots = bits1[word];
        for (uint32_t k = counts[2u * word + 1u]; roots && k < n1; ++k) {
            table1[k].first = word * 64u + comp_ctz(roots);
            roots &= roots - 1ull;
        }
    }
}

// a sum, a minimum, a maximum, flags: sent only where they change what a relaxed agent-scope load shows (the word only moves one way, so a value
// that has been overtaken costs an atomic that changes nothing, never a missing one)
__device__ __forceinline__ uint32_t stat_load(const uint32_t* at) { return __hip_atomic_load(at, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void stat_add(uint32_t* at, uint32_t v)
{
    if (v) (void)__hip_atomic_fetch_add(at, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ void stat_min(uint32_t* at, uint32_t v)
{
    if (v < stat_load(at)) (void)__hip_atomic_fetch_min(at, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ void stat_max(uint32_t* at, uint32_t v)
{
    if (v > stat_load(at)) (void)__hip_atomic_fetch_max(at, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ void stat_or(uint32_t* at, uint32_t v)
{
    if (v & ~stat_load(at)) (void)__hip_atomic_fetch_or(at, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// what a lane adds to a BoxStats: the voxels x0 .. x1 of row (y, z) with their flags; nothing (the neutral element of every field) where !has
struct BoxRun {
    uint32_t voxels, flags, lo[3], hi[3];
    __device__ __forceinline__ BoxRun(bool has, uint32_t count, uint32_t x0, uint32_t x1, uint32_t y, uint32_t z, uint32_t f)
        : voxels(has ? count : 0u), flags(has ? f : 0u), lo{has ? x0 : 0xffffffffu, has ? y : 0xffffffffu, has ? z : 0xffffffffu}, hi{has ? x1 : 0u, has ? y : 0u, has ? z : 0u}
    {
    }
    // every lane of the wave ends with the wave's total (every lane of the wave is here)
    __device__ __forceinline__ void reduce_wave()
    {
#pragma unroll
        for (uint32_t d = 1; d < 64u; d <<= 1) {
            voxels += (uint32_t)__shfl_xor((int)voxels, (int)d);
            flags |= (uint32_t)__shfl_xor((int)flags, (int)d);
#pragma unroll
            for (int a = 0; a < 3; ++a) lo[a] = min(lo[a], (uint32_t)__shfl_xor((int)lo[a], (int)d));
#pragma unroll
            for (int a = 0; a < 3; ++a) hi[a] = max(hi[a], (uint32_t)__shfl_xor((int)hi[a], (int)d));
        }
    }
    __device__ __forceinline__ void send(BoxStats* st) const
    {
        (void)__hip_atomic_fetch_add(&st->voxels, voxels, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);      // (a run that is sent has voxels)
#pragma unroll
        for (int a = 0; a < 3; ++a) stat_min(&st->lo[a], lo[a]);
#pragma unroll
        for (int a = 0; a < 3; ++a) stat_max(&st->hi[a], hi[a]);
        stat_or(&st->flags, flags);
    }
};

// Eight consecutive voxels per thread: two 16-byte loads of labels, one 8-byte load of the grid, a store only where a byte changed.  goes(label,
// state): whether the voxels of that label (never 0) leave, state = goes.prepare(), what a thread reads once; goes.becomes(): the byte (0 or 1)
// they turn into
template <class Goes> __global__ __launch_bounds__(256) void k_label_edit(uint8_t* grid, const uint32_t* __restrict__ labels, uint32_t groups, const Goes goes)
{
    const uint32_t t = blockIdx.x * 256u + threadIdx.x;
    if (t >= groups) return;
    const uint4 a = reinterpret_cast<const uint4*>(labels)[2u * (size_t)t], b = reinterpret_cast<const uint4*>(labels)[2u * (size_t)t + 1u];
    const uint32_t l[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
    if (!(a.x | a.y | a.z | a.w | b.x | b.y | b.z | b.w)) return;
    const uint32_t state = goes.prepare();
    uint64_t* at = reinterpret_cast<uint64_t*>(grid) + t;
    const uint64_t before = *at;
    uint64_t after = before;
#pragma unroll
    for (uint32_t k = 0; k < 8u; ++k)
        if (l[k] != 0u && goes(l[k], state)) after = (after & ~(0xffull << 8u * k)) | (goes.becomes() ? 1ull << 8u * k : 0ull);
    if (after != before) *at = after;
}

} // namespace dxv
