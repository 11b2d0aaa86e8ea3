// parity_lists.hip -- device build of the row lists of the parity rule (pl_rect, dxv_dirmap.h) from a scene's triangle records; their
// consumer is k_parity_rows, parity_rows.hip.
#include "dxv_device.h"
#include "dxv_dirmap.h"

namespace dxv {

namespace {
constexpr uint32_t kThreads = 256;

// ---------------------------------------------------------------------------------------------
// Row lists of the parity rule.  All its rays are +X lines: a row of voxels (fixed y, z) is one point of the (y, z)
// plane, and the triangles its rays can cross are those whose padded box covers that point (parity_row_setup's first
// test).  A grid of R x R texels over the plane lists per texel the triangles whose box reaches it: a row reads one
// 8-byte cell and then its candidates one after the other, instead of walking the tree to them (k_parity_rows waited on
// that chain of ~17 dependent node fetches per row).  A triangle is in a texel's list at most once, every candidate still
// takes the exact per-row test, and the order inside a list cannot matter to a count: the lists are filled through atomic
// cursors, without a sort.  Texels are a monotone function of the coordinate (dm_texel), the same on both sides.
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void k_pl_total(const TriPos* __restrict__ triPos, uint32_t T, uint32_t R, unsigned long long* __restrict__ total)
{
    // grid-stride: a few thousand waves, one pair of atomics each (one per wave of a 1 M-triangle launch on two addresses
    // was 0.3 ms of contention)
    unsigned long long n = 0, m = 0;                                   // entries; the largest rectangle of one triangle (a thread's loop in the fill)
    for (uint32_t t = blockIdx.x * kThreads + threadIdx.x; t < T; t += gridDim.x * kThreads) {
        uint32_t j0, j1, k0, k1;
        pl_rect(triPos[t], R, j0, j1, k0, k1);
        const unsigned long long r = (unsigned long long)(j1 - j0 + 1u) * (k1 - k0 + 1u);
        n += r;
        if (r > m) m = r;
    }
    for (int off = 32; off; off >>= 1) { n += __shfl_down(n, off); const unsigned long long o = __shfl_down(m, off); if (o > m) m = o; }
    if ((threadIdx.x & 63u) == 0u && n) { atomicAdd(total, n); atomicMax(total + 1, m); }
}
// FILL = false: counts[texel] += 1 per covered texel; FILL = true: entries[begin[texel] + cursor[texel]++] = triangle
template <bool FILL>
__global__ __launch_bounds__(kThreads) void k_pl_scatter(const TriPos* __restrict__ triPos, uint32_t T, uint32_t R, uint32_t* __restrict__ counts,
                                                         const uint32_t* __restrict__ begin, uint32_t* __restrict__ entries)
{
    const uint32_t t = blockIdx.x * kThreads + threadIdx.x;
    if (t >= T) return;
    uint32_t j0, j1, k0, k1;
    pl_rect(triPos[t], R, j0, j1, k0, k1);
    for (uint32_t k = k0; k <= k1; ++k) {
#pragma unroll 4
        for (uint32_t j = j0; j <= j1; ++j) {                           // (independent atomics: several in flight)
            const uint32_t c = k * R + j, slot = atomicAdd(counts + c, 1u);
            if (FILL) entries[begin[c] + slot] = t;
        }
    }
}
__global__ __launch_bounds__(kThreads) void k_pl_cells(const uint32_t* __restrict__ begin, const uint32_t* __restrict__ counts, uint32_t n, uint32_t* __restrict__ cells)
{
    const uint32_t c = blockIdx.x * kThreads + threadIdx.x;
    if (c < n) { cells[2u * c] = begin[c]; cells[2u * c + 1u] = counts[c]; }
}
} // namespace

__global__ __launch_bounds__(kThreads) void k_pl_validate(const uint32_t* __restrict__ cells, uint32_t ncells, const uint32_t* __restrict__ entries,
                                                          uint32_t n, uint32_t T, uint32_t* __restrict__ out)
{
    uint32_t badCells = 0, badTris = 0;
    for (uint32_t c = blockIdx.x * kThreads + threadIdx.x; c < ncells; c += gridDim.x * kThreads)
        if (cells[2u * c + 1u] && ((uint64_t)cells[2u * c] + cells[2u * c + 1u] > (uint64_t)n)) ++badCells;
    for (uint32_t i = blockIdx.x * kThreads + threadIdx.x; i < n; i += gridDim.x * kThreads)
        if (entries[i] >= T) ++badTris;
    if (badCells) atomicAdd(out, badCells);
    if (badTris) atomicAdd(out + 1, badTris);
}
hipError_t parity_lists_validate(const uint32_t* cells, uint32_t R, const uint32_t* entries, uint32_t n, uint32_t T, uint32_t* out, hipStream_t s)
{
    hipError_t e = hipMemsetAsync(out, 0, 2 * sizeof(uint32_t), s);
    if (e != hipSuccess) return e;
    k_pl_validate<<<1024, kThreads, 0, s>>>(cells, R * R, entries, n, T, out);
    return hipGetLastError();
}

// The lists (above).  parity_lists_total: total[0] = entries the lists would have, total[1] = texels of the
// largest single rectangle (one thread of the fill walks it); parity_lists_fill: cells = 2 words
// (begin, count) per texel of the R x R grid, entries = `total` triangle slots (+ a few spare words behind them).
// counts / offsets: R R words each, sums: ceil(R R / 1024) + 1 words of scratch.
hipError_t parity_lists_total(const TriPos* triPos, uint32_t T, uint32_t R, unsigned long long* total, hipStream_t s)
{
    hipError_t e = hipMemsetAsync(total, 0, 2 * sizeof(unsigned long long), s);
    if (e != hipSuccess) return e;
    const uint32_t blocks = (T + kThreads - 1) / kThreads;
    k_pl_total<<<blocks < 512u ? blocks : 512u, kThreads, 0, s>>>(triPos, T, R, total);
    return hipGetLastError();
}
hipError_t parity_lists_fill(const TriPos* triPos, uint32_t T, uint32_t R, uint32_t* counts, uint32_t* offsets, uint32_t* sums, uint32_t* cells,
                             uint32_t* entries, hipStream_t s)
{
    const uint32_t n = R * R, blocks = (T + kThreads - 1) / kThreads;
    hipError_t e;
    if ((e = hipMemsetAsync(counts, 0, sizeof(uint32_t) * n, s)) != hipSuccess) return e;
    k_pl_scatter<false><<<blocks, kThreads, 0, s>>>(triPos, T, R, counts, nullptr, nullptr);
    if ((e = scan_exclusive(counts, n, sums, offsets, s)) != hipSuccess) return e;
    if ((e = hipMemsetAsync(counts, 0, sizeof(uint32_t) * n, s)) != hipSuccess) return e;
    k_pl_scatter<true><<<blocks, kThreads, 0, s>>>(triPos, T, R, counts, offsets, entries);
    k_pl_cells<<<(n + kThreads - 1) / kThreads, kThreads, 0, s>>>(offsets, counts, n, cells);
    return hipGetLastError();
}

} // namespace dxv
