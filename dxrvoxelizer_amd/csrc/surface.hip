// surface.hip -- the surface rule (DXV_MODE_SURFACE; the shell of DXV_MODE_REFERENCE_SURFACE), DESIGN.md §2 and §4: a triangle-parallel
// scatter over the scene's triangle records into a partition that the launch has cleared (mode 2) or that holds the reference rule's
// grid (mode 3).  It reads nothing but triPos, so every kind of scene has it: static, refitted, imported, with or without lists.
//   k_surface_tris:  one lane per triangle.  A triangle whose candidate box (dxv_surface.h: surface_box) holds at most kSurfaceSmall
//                    voxels is tested voxel by voxel by its lane; a larger one is cut into work items of kSurfaceChunkCols columns of
//                    its projection onto its dominant axis plane, appended to the frame's own list (or, if that is full, listed whole).
//   k_surface_large: one 64-lane workgroup per work item (or whole triangle) at a time, a lane per column: only the columns whose square (widened) meets
//                    the projected triangle, and in each only the depths the triangle's plane can reach (widened by one voxel); every
//                    column over its whole depth range for a triangle with a vertex so far outside the grid that the float32 test no
//                    longer follows the exact plane to within those margins (dxv_surface.h: kSurfaceFar, derived there).
// Every test is the canonical one (surface_overlap); the enumerations (dxv_surface.h: tri_box, box_is_small, cols_setup, column_range --
// host-callable, tests/hostcheck/surface_check.cpp runs them on the CPU) have to be supersets of what it accepts, whichever of the two
// paths the partition's z clip sends a triangle down.  Writes are plain byte stores of 1:
// two triangles that share a voxel store the same value, no atomics are needed for the grid.
#include "dxv_device.h"
#include "dxv_surface.h"

#pragma clang fp contract(off)

namespace dxv {

constexpr uint32_t kSurfaceChunkCols = 256;   // columns per work item of the large path (64 lanes, four columns each)
constexpr uint32_t kSurfaceGroups = 2048;     // persistent workgroups of k_surface_large (eight waves per CU)
constexpr uint32_t kSurfaceItems = 1u << 20;  // work items the list holds (a triangle whose items do not all fit is listed whole as well)

size_t surface_scratch_bytes(uint32_t T) { return 256u + sizeof(uint32_t) * (2u * (size_t)kSurfaceItems + T); }

__device__ inline SurfaceTri load_tri(const TriPos* __restrict__ triPos, uint32_t t)
{
    const TriPos q = triPos[t];
    return SurfaceTri{{q.v0.x, q.v0.y, q.v0.z}, {q.v1.x, q.v1.y, q.v1.z}, {q.v2.x, q.v2.y, q.v2.z}};
}

__device__ inline void test_voxel(const SurfaceGrid& g, const SurfaceTri& t, int ix, int iy, int iz, uint32_t lz)
{
    float cx, cy, cz;
    ray_origin(g.N, (uint32_t)ix, (uint32_t)iy, (uint32_t)iz, cx, cy, cz);
    if (surface_overlap(t.a, t.b, t.d, cx, cy, cz, g.h)) g.grid[((size_t)lz * g.N + (uint32_t)iy) * g.N + (uint32_t)ix] = 1;
}

// column `col` of the box's (u, v) rectangle (dxv_surface.h: column_range): skipped, or tested over the depths it is given
__device__ inline void walk_column(const SurfaceGrid& g, const SurfaceTri& t, const SurfaceCols& s, uint32_t col)
{
    int iu, iv, k0, k1;
    if (!column_range(s, col, iu, iv, k0, k1)) return;
#pragma clang loop unroll(disable)
    for (int k = k0; k <= k1; ++k) {
        int x, y, z;
        column_voxel(s, iu, iv, k, x, y, z);
        uint32_t lz;
        if (local_slice(g, z, lz)) test_voxel(g, t, x, y, z, lz);
    }
}

// scratch of the pass (surface_scratch_bytes): [0] work items listed (64 bit), [2] triangles listed whole; from byte 256 the work
// items (triangle, chunk), then the triangles listed whole (those that found the item list full: at most T)
__global__ __launch_bounds__(256) void k_surface_tris(const TriPos* __restrict__ triPos, uint32_t T, SurfaceGrid g, uint32_t* __restrict__ scratch)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= T) return;
    const SurfaceTri t = load_tri(triPos, i);
    int lo[3], hi[3];
    if (!tri_box(g, t, lo, hi)) return;
    if (box_is_small(lo, hi)) {
        const uint32_t nx = (uint32_t)(hi[0] - lo[0] + 1), ny = (uint32_t)(hi[1] - lo[1] + 1), nz = (uint32_t)(hi[2] - lo[2] + 1);
        // (one voxel per iteration: unrolled copies of the test only cost registers)
        int x = lo[0], y = lo[1], z = lo[2];
#pragma clang loop unroll(disable)
        for (uint32_t k = 0; k < nx * ny * nz; ++k) {
            uint32_t lz;
            if (local_slice(g, z, lz)) test_voxel(g, t, x, y, z, lz);
            if (++x > hi[0]) { x = lo[0]; if (++y > hi[1]) { y = lo[1]; ++z; } }
        }
        return;
    }
    SurfaceCols s;
    cols_setup(g, t, lo, hi, s);
    const uint32_t chunks = (s.cols + kSurfaceChunkCols - 1u) / kSurfaceChunkCols;
    const unsigned long long slot = atomicAdd(reinterpret_cast<unsigned long long*>(scratch), (unsigned long long)chunks);
    uint32_t* items = scratch + 64;
    // k_surface_large reads every slot below min(listed, items): each one a reservation took is written here, by the triangle that
    // took it -- also when the reservation runs past the end.  A triangle whose items do not all fit is listed whole as well (the
    // columns it walks twice store the same 1s).
    for (uint32_t c = 0; c < chunks && slot + c < g.items; ++c) {
        items[2u * (slot + c)] = i;
        items[2u * (slot + c) + 1u] = c;
    }
    if (slot + chunks > g.items) {
        const uint32_t w = atomicAdd(scratch + 2, 1u);             // (< T: a triangle is listed once)
        items[2u * kSurfaceItems + w] = i;
    }
}

__device__ inline void large_item(const TriPos* __restrict__ triPos, uint32_t T, const SurfaceGrid& g, uint32_t tri, uint32_t colFirst, uint32_t colEnd)
{
    if (tri >= T) return;                                          // (every item read was written by this launch: a guard, not a path)
    const SurfaceTri t = load_tri(triPos, tri);
    int lo[3], hi[3];
    if (!tri_box(g, t, lo, hi)) return;
    SurfaceCols s;
    cols_setup(g, t, lo, hi, s);
    const uint32_t end = colEnd < s.cols ? colEnd : s.cols;
    for (uint32_t col = colFirst + threadIdx.x; col < end; col += 64u) walk_column(g, t, s, col);
}

__global__ __launch_bounds__(64) void k_surface_large(const TriPos* __restrict__ triPos, uint32_t T, SurfaceGrid g, const uint32_t* __restrict__ scratch)
{
    const unsigned long long listed = *reinterpret_cast<const unsigned long long*>(scratch);
    const uint32_t n = listed < g.items ? (uint32_t)listed : g.items;
    const uint32_t whole = min(scratch[2], T);
    const uint32_t* items = scratch + 64;
    for (uint32_t r = blockIdx.x; r < n; r += gridDim.x) {
        const uint32_t chunk = items[2u * r + 1u];
        large_item(triPos, T, g, items[2u * r], chunk * kSurfaceChunkCols, (chunk + 1u) * kSurfaceChunkCols);
    }
    for (uint32_t r = blockIdx.x; r < whole; r += gridDim.x) large_item(triPos, T, g, items[2u * kSurfaceItems + r], 0u, 0xffffffffu);
}

hipError_t launch_surface(const SurfaceParams& p, hipStream_t s)
{
    if (!p.T || !p.nz) return hipSuccess;
    SurfaceGrid g{};
    g.grid = p.grid; g.N = p.N; g.z0 = p.z0; g.nz = p.nz; g.zBlock = p.zBlock; g.zPeriod = p.zPeriod;
    g.zLast = p.z0 + ((p.nz - 1u) / p.zBlock) * p.zPeriod + (p.nz - 1u) % p.zBlock;
    g.h = 1.0f / (float)p.N;
    g.items = p.items && p.items < kSurfaceItems ? p.items : kSurfaceItems;
    uint32_t* scratch = reinterpret_cast<uint32_t*>(p.scratch);
    const hipError_t e = hipMemsetAsync(scratch, 0, 4u * sizeof(uint32_t), s);
    if (e != hipSuccess) return e;
    k_surface_tris<<<(p.T + 255u) / 256u, 256, 0, s>>>(p.triPos, p.T, g, scratch);
    k_surface_large<<<kSurfaceGroups, 64, 0, s>>>(p.triPos, p.T, g, scratch);
    return hipGetLastError();
}

}  // namespace dxv
