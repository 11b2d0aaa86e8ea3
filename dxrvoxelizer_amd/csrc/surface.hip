// surface.hip -- the surface rule (DXV_MODE_SURFACE; the shell of DXV_MODE_REFERENCE_SURFACE), DESIGN.md §2 and §4: a triangle-parallel
// scatter over the scene's triangle records into a partition that the launch has cleared (mode 2) or that holds the reference rule's
// grid (mode 3).  It reads nothing but triPos, so every kind of scene has it: static, refitted, imported, with or without lists.
//   k_surface_tris:  one lane per triangle.  A triangle whose candidate box (dxv_surface.h: surface_box) holds at most kSurfaceSmall
//                    voxels is tested voxel by voxel by its lane; a larger one is cut into work items of kSurfaceChunkCols columns of
//                    its projection onto its dominant axis plane, appended to the frame's own list (or, if that is full, listed whole).
//   k_surface_large: one 64-lane workgroup per work item (or whole triangle) at a time, a lane per column: only the columns whose square (widened) meets
//                    the projected triangle, and in each only the depths the triangle's plane can reach (widened by one voxel).
// Every test is the canonical one (surface_overlap); the enumerations only have to be supersets.  Writes are plain byte stores of 1:
// two triangles that share a voxel store the same value, no atomics are needed for the grid.
#include "dxv_device.h"
#include "dxv_surface.h"

#pragma clang fp contract(off)

namespace dxv {

constexpr uint32_t kSurfaceSmall = 64;        // candidate voxels a lane tests on its own
constexpr uint32_t kSurfaceChunkCols = 256;   // columns per work item of the large path (64 lanes, four columns each)
constexpr uint32_t kSurfaceGroups = 2048;     // persistent workgroups of k_surface_large (eight waves per CU)
constexpr uint32_t kSurfaceItems = 1u << 20;  // work items the list holds (a triangle whose items do not all fit is listed whole as well)

size_t surface_scratch_bytes(uint32_t T) { return 256u + sizeof(uint32_t) * (2u * (size_t)kSurfaceItems + T); }

struct SurfaceGrid {
    uint8_t* grid;
    uint32_t N, z0, nz, zBlock, zPeriod, zLast;     // zLast: the partition's last global slice
    float h;                                        // half a voxel, 1.0f / N
    uint32_t items;                                 // work items the list may take (kSurfaceItems; fewer under option surfaceitems)
};

struct SurfaceTri { float a[3], b[3], d[3]; };

__device__ inline SurfaceTri load_tri(const TriPos* __restrict__ triPos, uint32_t t)
{
    const TriPos q = triPos[t];
    return SurfaceTri{{q.v0.x, q.v0.y, q.v0.z}, {q.v1.x, q.v1.y, q.v1.z}, {q.v2.x, q.v2.y, q.v2.z}};
}

// the candidate box, its z range clipped to the partition's first and last slice
__device__ inline bool tri_box(const SurfaceGrid& g, const SurfaceTri& t, int lo[3], int hi[3])
{
    if (!surface_box(t.a, t.b, t.d, g.N, lo, hi)) return false;
    lo[2] = max(lo[2], (int)g.z0);
    hi[2] = min(hi[2], (int)g.zLast);
    return lo[2] <= hi[2];
}

// global slice z (z0 <= z <= zLast) -> local slice of the partition, or false when the partition does not hold it
__device__ inline bool local_slice(const SurfaceGrid& g, int z, uint32_t& lz)
{
    const uint32_t dz = (uint32_t)z - g.z0, q = dz / g.zPeriod, r = dz - q * g.zPeriod;
    lz = q * g.zBlock + r;
    return r < g.zBlock && lz < g.nz;
}

__device__ inline void test_voxel(const SurfaceGrid& g, const SurfaceTri& t, int ix, int iy, int iz, uint32_t lz)
{
    float cx, cy, cz;
    ray_origin(g.N, (uint32_t)ix, (uint32_t)iy, (uint32_t)iz, cx, cy, cz);
    if (surface_overlap(t.a, t.b, t.d, cx, cy, cz, g.h)) g.grid[((size_t)lz * g.N + (uint32_t)iy) * g.N + (uint32_t)ix] = 1;
}

// Column set-up of the large path, in voxel units and double precision (the triangle's plane decides which depths a column tests;
// a plane made of rounded float products could be far off for a sliver), with the axes renamed: w = the normal's dominant axis,
// (u, v) = (w + 1, w + 2) mod 3 the plane the triangle is projected onto.
struct SurfaceCols {
    double au, av, aw, bu, bv, du, dv;   // the vertices' (u, v) and a's depth
    double nu, nv, nw;                   // the normal
    int w, u0, v0, w0, w1, rowCols;      // box: columns from (u0, v0), rowCols of them per row, depths [w0, w1]
    uint32_t cols;
    bool plane;                          // false: (nearly) degenerate -- every column tests its whole depth range in the box
};

__device__ inline double vox(float p, int k, double half) { return k == 1 ? (1.0 - (double)p) * half : ((double)p + 1.0) * half; }

__device__ inline void cols_setup(const SurfaceGrid& g, const SurfaceTri& t, const int lo[3], const int hi[3], SurfaceCols& s)
{
    const double half = 0.5 * (double)g.N;
    const double A[3] = {vox(t.a[0], 0, half), vox(t.a[1], 1, half), vox(t.a[2], 2, half)};
    const double B[3] = {vox(t.b[0], 0, half), vox(t.b[1], 1, half), vox(t.b[2], 2, half)};
    const double D[3] = {vox(t.d[0], 0, half), vox(t.d[1], 1, half), vox(t.d[2], 2, half)};
    const double e1x = B[0] - A[0], e1y = B[1] - A[1], e1z = B[2] - A[2];
    const double e2x = D[0] - A[0], e2y = D[1] - A[1], e2z = D[2] - A[2];
    const double nx = e1y * e2z - e1z * e2y, ny = e1z * e2x - e1x * e2z, nz = e1x * e2y - e1y * e2x;
    const double ax = fabs(nx), ay = fabs(ny), az = fabs(nz);
    const int w = (ax >= ay && ax >= az) ? 0 : (ay >= az ? 1 : 2);
    // (u, v) = (y, z), (z, x), (x, y) for w = x, y, z
    s.w = w;
    s.au = w == 0 ? A[1] : (w == 1 ? A[2] : A[0]);  s.av = w == 0 ? A[2] : (w == 1 ? A[0] : A[1]);  s.aw = w == 0 ? A[0] : (w == 1 ? A[1] : A[2]);
    s.bu = w == 0 ? B[1] : (w == 1 ? B[2] : B[0]);  s.bv = w == 0 ? B[2] : (w == 1 ? B[0] : B[1]);
    s.du = w == 0 ? D[1] : (w == 1 ? D[2] : D[0]);  s.dv = w == 0 ? D[2] : (w == 1 ? D[0] : D[1]);
    s.nu = w == 0 ? ny : (w == 1 ? nz : nx);        s.nv = w == 0 ? nz : (w == 1 ? nx : ny);        s.nw = w == 0 ? nx : (w == 1 ? ny : nz);
    const int u0 = w == 0 ? lo[1] : (w == 1 ? lo[2] : lo[0]), u1 = w == 0 ? hi[1] : (w == 1 ? hi[2] : hi[0]);
    const int v0 = w == 0 ? lo[2] : (w == 1 ? lo[0] : lo[1]), v1 = w == 0 ? hi[2] : (w == 1 ? hi[0] : hi[1]);
    s.u0 = u0; s.v0 = v0;
    s.w0 = w == 0 ? lo[0] : (w == 1 ? lo[1] : lo[2]);
    s.w1 = w == 0 ? hi[0] : (w == 1 ? hi[1] : hi[2]);
    const double l1 = fmax(fabs(e1x), fmax(fabs(e1y), fabs(e1z))), l2 = fmax(fabs(e2x), fmax(fabs(e2y), fabs(e2z)));
    s.plane = fabs(s.nw) > 1e-9 * l1 * l2;
    s.rowCols = u1 - u0 + 1;
    s.cols = (uint32_t)s.rowCols * (uint32_t)(v1 - v0 + 1);
}

// one edge of the projected triangle against a column's square of half size 1 (the column's own square widened by half a voxel)
__device__ inline bool edge2_separates(double pu, double pv, double qu, double qv, const SurfaceCols& s, double cu, double cv)
{
    const double gu = pv - qv, gv = qu - pu;
    const double pa = gu * s.au + gv * s.av, pb = gu * s.bu + gv * s.bv, pd = gu * s.du + gv * s.dv;
    const double c = gu * cu + gv * cv, r = fabs(gu) + fabs(gv);
    return fmin(pa, fmin(pb, pd)) > c + r || fmax(pa, fmax(pb, pd)) < c - r;
}

// column `col` of the box's (u, v) rectangle: skipped unless its widened square meets the projected triangle; then the depths the
// plane reaches over the square, one voxel more on either side, clipped to the box
__device__ inline void walk_column(const SurfaceGrid& g, const SurfaceTri& t, const SurfaceCols& s, uint32_t col)
{
    const int iu = s.u0 + (int)(col % (uint32_t)s.rowCols), iv = s.v0 + (int)(col / (uint32_t)s.rowCols);
    const double cu = (double)iu + 0.5, cv = (double)iv + 0.5;
    if (edge2_separates(s.au, s.av, s.bu, s.bv, s, cu, cv) || edge2_separates(s.bu, s.bv, s.du, s.dv, s, cu, cv) ||
        edge2_separates(s.du, s.dv, s.au, s.av, s, cu, cv))
        return;
    int k0 = s.w0, k1 = s.w1;
    if (s.plane) {
        const double wc = s.aw - (s.nu * (cu - s.au) + s.nv * (cv - s.av)) / s.nw;
        const double sp = 0.5 * (fabs(s.nu) + fabs(s.nv)) / fabs(s.nw);
        // (clamped into [w0 - 1, w1 + 1] before the conversion; a NaN leaves the whole range)
        k0 = (int)fmin(fmax(floor(wc - sp) - 1.0, (double)s.w0), (double)s.w1 + 1.0);
        k1 = (int)fmax(fmin(floor(wc + sp) + 1.0, (double)s.w1), (double)s.w0 - 1.0);
    }
#pragma clang loop unroll(disable)
    for (int k = k0; k <= k1; ++k) {
        const int x = s.w == 0 ? k : (s.w == 1 ? iv : iu);
        const int y = s.w == 0 ? iu : (s.w == 1 ? k : iv);
        const int z = s.w == 0 ? iv : (s.w == 1 ? iu : k);
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
    const uint32_t nx = (uint32_t)(hi[0] - lo[0] + 1), ny = (uint32_t)(hi[1] - lo[1] + 1), nz = (uint32_t)(hi[2] - lo[2] + 1);
    if ((uint64_t)nx * ny * nz <= kSurfaceSmall) {
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
