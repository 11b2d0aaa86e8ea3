// thickness.hip -- the exact local thickness of a whole N^3 grid (dxv_thickness.h has the rule and the routines of every stage), on the frame's
// stream.  A fixed chain of kernels; every count a later kernel needs stays in device memory.
//   field      distance.hip: F = DXV_DIST_SQ_I32 of the grid, into the operator's own buffer
//   k_thick_members   F -> E = { R == cap } as bytes, four voxels per thread
//   top        distance.hip of E, then k_thick_top: E and its field -> Top as bytes (in place) and the start of W: cap on Top, R elsewhere
//   cull       distance.hip of Top (option thickcull bit 0)
//   k_thick_select    per block of 1024 voxels: the work items of every voxel (0: no centre to paint) as a byte, the block's centres and items;
//                     it also zeroes the two words behind the totals that the paint counts in
//   scan.hip          launch_scan_sums, one workgroup: the exclusive scan of the blocks' two sums, 64-bit, and the totals behind them
//   k_thick_emit      the scan inside every block: the compacted centre list (voxel index) and every centre's first item within its block
//   k_thick_paint     a fixed launch of waves striding over the items: item -> block -> centre by two binary searches (wave-uniform), then the
//                     slice of the ball in row order, lanes along x: a plain load of W and a relaxed atomic max without return only where the
//                     loaded value is lower.  W only grows, so a stale load costs a spare atomic and never loses one.
//   k_thick_histogram W -> cap + 1 64-bit bins through 32-bit bins in LDS (16.4 KB), one 64-bit atomic per non-zero bin and workgroup
// No kernel waits for another workgroup, no loop is unbounded, nothing goes to scratch memory; LDS: the histogram's bins and the four wave sums
// of a block's scan (dxv_scan.h).  The scratch is laid out by thickness_carve (dxv_thickness.h).
#include "dxv_device.h"
#include "dxv_thickness.h"
#include "dxv_scan.h"

namespace dxv {

constexpr uint32_t kThickPaintBlocks = 2048;      // workgroups of four waves the paint is launched with, whatever the items
constexpr uint32_t kThickHistBlocks = 1024;       // ... the histogram, at the most

__global__ __launch_bounds__(256) void k_thick_members(const int32_t* __restrict__ F, uint32_t groups, int of, uint32_t cap, uint32_t* __restrict__ B)
{
    const uint32_t t = blockIdx.x * 256u + threadIdx.x;
    if (t >= groups) return;
    const int4 d = reinterpret_cast<const int4*>(F)[t];
    B[t] = (thick_radius(d.x, of, cap) == cap ? 1u : 0u) | (thick_radius(d.y, of, cap) == cap ? 1u << 8 : 0u) | (thick_radius(d.z, of, cap) == cap ? 1u << 16 : 0u) |
           (thick_radius(d.w, of, cap) == cap ? 1u << 24 : 0u);
}

__global__ __launch_bounds__(256) void k_thick_top(const int32_t* __restrict__ F, const int32_t* __restrict__ dE, uint32_t groups, int of, uint32_t cap, uint32_t* __restrict__ B,
                                                   uint32_t* __restrict__ W)
{
    const uint32_t t = blockIdx.x * 256u + threadIdx.x;
    if (t >= groups) return;
    const int4 d = reinterpret_cast<const int4*>(F)[t], e = reinterpret_cast<const int4*>(dE)[t];
    const uint32_t b = B[t];
    const uint32_t t0 = thick_top(b & 0xffu, e.x, cap), t1 = thick_top((b >> 8) & 0xffu, e.y, cap), t2 = thick_top((b >> 16) & 0xffu, e.z, cap), t3 = thick_top(b >> 24, e.w, cap);
    B[t] = t0 | t1 << 8 | t2 << 16 | t3 << 24;
    reinterpret_cast<uint4*>(W)[t] = make_uint4(t0 ? cap : thick_radius(d.x, of, cap), t1 ? cap : thick_radius(d.y, of, cap), t2 ? cap : thick_radius(d.z, of, cap),
                                                t3 ? cap : thick_radius(d.w, of, cap));
}

// thread t of block b: voxels 1024 b + 4 t .. + 3 (N^3 is a multiple of 8: the four are all inside or all outside).  A block's centres (above bit
// 20) and items (below it) are scanned in one word: at most 1024 and 1024 * 127.  Thread 0 of block 0 also zeroes the two words behind the totals
// that k_thick_paint<true> counts in: this kernel is the first of the select stage, the paint is a later stage of the same stream, and nothing
// between the two -- the scan of the sums writes the blocks' entries and the two totals, k_thick_emit only reads the sums -- touches those words.
__global__ __launch_bounds__(256) void k_thick_select(ThickParams p, uint32_t voxels)
{
    if (blockIdx.x == 0 && threadIdx.x == 0) { p.sums[2 * (size_t)gridDim.x + 2] = 0; p.sums[2 * (size_t)gridDim.x + 3] = 0; }
    const uint32_t first = blockIdx.x * kThickBlock + threadIdx.x * 4u;
    uint32_t bytes = 0, mine = 0;
    if (first < voxels) {
        const uint32_t N = p.N, row = first / N;
        uint32_t x = first - row * N, y = row % N, z = row / N;
#pragma unroll
        for (uint32_t k = 0; k < 4u; ++k) {
            const uint32_t items = thick_items(p.F, p.G, N, x, y, z, p.of, p.cap, p.cull);
            bytes |= items << 8u * k;
            mine += items ? (1u << 20) + items : 0u;
            if (++x == N) { x = 0; if (++y == N) { y = 0; ++z; } }
        }
        p.B[first >> 2] = bytes;
    }
    uint32_t total;
    (void)block_scan_exclusive<uint32_t, 4>(mine, total);
    if (threadIdx.x == 0) { p.sums[2 * (size_t)blockIdx.x] = total >> 20; p.sums[2 * (size_t)blockIdx.x + 1] = total & 0xfffffu; }
}

__global__ __launch_bounds__(256) void k_thick_emit(ThickParams p, uint32_t voxels)
{
    const uint32_t first = blockIdx.x * kThickBlock + threadIdx.x * 4u;
    const uint32_t bytes = first < voxels ? p.B[first >> 2] : 0u;
    uint32_t mine = 0;
#pragma unroll
    for (uint32_t k = 0; k < 4u; ++k) {
        const uint32_t items = (bytes >> 8u * k) & 0xffu;
        mine += items ? (1u << 20) + items : 0u;
    }
    uint32_t total;
    uint32_t run = block_scan_exclusive<uint32_t, 4>(mine, total);
    if (!mine) return;
    const size_t base = (size_t)p.sums[2 * (size_t)blockIdx.x];         // (at most N^3 centres: below 2^30)
#pragma unroll
    for (uint32_t k = 0; k < 4u; ++k) {
        const uint32_t items = (bytes >> 8u * k) & 0xffu;
        if (!items) continue;
        p.centres[base + (run >> 20)] = first + k;
        p.firstItem[base + (run >> 20)] = run & 0xfffffu;
        run += (1u << 20) + items;
    }
}

// kCount: the measurement build of the same paint (option thickstages), which also counts the voxels it tests and the atomics it sends
template <bool kCount> __global__ __launch_bounds__(256) void k_thick_paint(ThickParams p, uint32_t blocks)
{
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wave = blockIdx.x * 4u + (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), waves = gridDim.x * 4u;
    const unsigned long long* sums = p.sums;
    const unsigned long long total = sums[2 * (size_t)blocks + 1];
    const uint32_t N = p.N;
    unsigned long long tested = 0, sent = 0;
    for (unsigned long long i = wave; i < total; i += waves) {
        uint32_t lo = 0, hi = blocks;                                   // the last block whose first item is <= i: the one that holds it
        while (hi - lo > 1u) {
            const uint32_t mid = lo + (hi - lo) / 2u;
            if (sums[2 * (size_t)mid + 1] <= i) lo = mid; else hi = mid;
        }
        const uint32_t local = (uint32_t)(i - sums[2 * (size_t)lo + 1]);
        uint32_t a = (uint32_t)sums[2 * (size_t)lo], b = (uint32_t)sums[2 * (size_t)lo + 2];   // the block's centres [a, b): not empty, it holds an item
        while (b - a > 1u) {
            const uint32_t mid = a + (b - a) / 2u;
            if (p.firstItem[mid] <= local) a = mid; else b = mid;
        }
        const uint32_t v = p.centres[a], k = local - p.firstItem[a];
        if (v >= N * N * N) continue;                                   // (never: what k_thick_emit wrote is a voxel of the grid)
        const uint32_t row = v / N, x = v - row * N, y = row % N, z = row / N;
        const uint32_t R = thick_radius(p.F[v], p.of, p.cap), h = thick_reach(R < 1u ? 1u : R);
        if (R < 2u || k >= thick_discs(z, h, N)) continue;              // (never, for the same reason: no write leaves the ball or the grid)
        uint32_t* W = p.W;
        thick_paint_disc(N, x, y, z, R, thick_disc_first(z, h) + k, lane, 64u, [W, &tested, &sent](size_t at, uint32_t r) {
            if (kCount) ++tested;
            if (W[at] < r) { if (kCount) ++sent; (void)__hip_atomic_fetch_max(W + at, r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
        });
    }
    if (!kCount) return;
    // what the wave did, for dxv_thickness_stage_info: one pair of atomics per wave, behind the totals
#pragma unroll
    for (uint32_t d = 1; d < 64u; d <<= 1) { tested += __shfl_xor(tested, d); sent += __shfl_xor(sent, d); }
    if (lane == 0u && tested) {
        (void)__hip_atomic_fetch_add(p.sums + 2 * (size_t)blocks + 2, tested, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (sent) (void)__hip_atomic_fetch_add(p.sums + 2 * (size_t)blocks + 3, sent, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

__global__ __launch_bounds__(256) void k_thick_histogram(const uint32_t* __restrict__ W, uint32_t groups, uint32_t cap, unsigned long long* __restrict__ hist)
{
    __shared__ uint32_t bins[kThickMaxCapSq + 1u];                      // (a workgroup counts fewer than 2^32 voxels: N^3 <= 2^30)
    for (uint32_t t = threadIdx.x; t <= cap; t += 256u) bins[t] = 0u;
    __syncthreads();
    for (uint32_t g = blockIdx.x * 256u + threadIdx.x; g < groups; g += gridDim.x * 256u) {
        const uint4 w = reinterpret_cast<const uint4*>(W)[g];
        atomicAdd(&bins[w.x <= cap ? w.x : cap], 1u);                   // (W <= cap: the clamp keeps a damaged field inside the bins)
        atomicAdd(&bins[w.y <= cap ? w.y : cap], 1u);
        atomicAdd(&bins[w.z <= cap ? w.z : cap], 1u);
        atomicAdd(&bins[w.w <= cap ? w.w : cap], 1u);
    }
    __syncthreads();
    for (uint32_t t = threadIdx.x; t <= cap; t += 256u)
        if (bins[t]) (void)__hip_atomic_fetch_add(hist + t, (unsigned long long)bins[t], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

size_t thickness_histogram_bytes(uint32_t cap) { return ((size_t)cap + 1u) * sizeof(unsigned long long); }

static bool thick_valid(const uint8_t* grid, const ThickParams& p)
{
    return grid && p.F && p.W && p.hist && p.N >= 2u && p.N <= kThickMaxN && !(p.N & 1u) && (p.of == THICK_SOLID || p.of == THICK_EMPTY) && p.cap >= kThickMinCapSq &&
           p.cap <= kThickMaxCapSq && p.cull <= 3u;
}

hipError_t launch_thickness_stage(const uint8_t* grid, const ThickParams& p, int stage, hipStream_t s)
{
    if (!thick_valid(grid, p)) return hipErrorInvalidValue;
    const uint32_t N = p.N, voxels = N * N * N, groups = voxels / 4u, blocks = thick_blocks(N);
    hipError_t e = hipSuccess;
    switch (stage) {
    case THICK_STAGE_FIELD:
        return launch_distance(grid, N, 0, p.F, p.passes, s);
    case THICK_STAGE_TOP:
        k_thick_members<<<(groups + 255u) / 256u, 256, 0, s>>>(p.F, groups, p.of, p.cap, p.B);
        if ((e = launch_distance(reinterpret_cast<const uint8_t*>(p.B), N, 0, p.G, p.passes, s)) != hipSuccess) return e;
        k_thick_top<<<(groups + 255u) / 256u, 256, 0, s>>>(p.F, p.G, groups, p.of, p.cap, p.B, p.W);
        break;
    case THICK_STAGE_CULL:
        if (p.cull & THICK_CULL_TOP) return launch_distance(reinterpret_cast<const uint8_t*>(p.B), N, 0, p.G, p.passes, s);
        break;
    case THICK_STAGE_SELECT:
        k_thick_select<<<blocks, 256, 0, s>>>(p, voxels);
        if ((e = launch_scan_sums(p.sums, 2, blocks, p.sums + 2 * (size_t)blocks, s)) != hipSuccess) return e;
        k_thick_emit<<<blocks, 256, 0, s>>>(p, voxels);
        break;
    case THICK_STAGE_PAINT:
        if (p.count) k_thick_paint<true><<<kThickPaintBlocks, 256, 0, s>>>(p, blocks);
        else k_thick_paint<false><<<kThickPaintBlocks, 256, 0, s>>>(p, blocks);
        break;
    case THICK_STAGE_HISTOGRAM: {
        if ((e = hipMemsetAsync(p.hist, 0, thickness_histogram_bytes(p.cap), s)) != hipSuccess) return e;
        const uint32_t want = (groups + 255u) / 256u;
        k_thick_histogram<<<want < kThickHistBlocks ? want : kThickHistBlocks, 256, 0, s>>>(p.W, groups, p.cap, p.hist);
        break;
    }
    default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

} // namespace dxv
