// dxv_surface.h -- the surface rule (DXV_MODE_SURFACE): voxel (ix, iy, iz) is set when its CLOSED box overlaps the
// CLOSED triangle.  Akenine-Möller's triangle-box separating-axis test, float32 in the fixed order DESIGN §2 writes down (no
// contraction: the translation units that include this file are built with -ffp-contract=off), so that tests/surface_restated.py
// restates it bit for bit.  The candidate enumeration helpers below only have to give a superset of the voxels the test accepts.
#pragma once
#include "dxv_math.h"

#pragma clang fp contract(off)

namespace dxv {

DXV_HD float min3_(float a, float b, float c) { return min_(min_(a, b), c); }
DXV_HD float max3_(float a, float b, float c) { return max_(max_(a, b), c); }

// edge axis e x unit(i), (j, k) = (i+1, i+2) mod 3: all three vertices projected (no rounding case depends on which two own the edge)
DXV_HD bool surface_edge_separates(float ej, float ek, float v0j, float v0k, float v1j, float v1k, float v2j, float v2k, float h)
{
    const float p0 = ej * v0k - ek * v0j;
    const float p1 = ej * v1k - ek * v1j;
    const float p2 = ej * v2k - ek * v2j;
    const float r = abs_(ej) * h + abs_(ek) * h;
    return min3_(p0, p1, p2) > r || max3_(p0, p1, p2) < -r;
}

// the canonical test: triangle (a, b, d) in the scene's normalised space, box centre (cx, cy, cz) = the ray rule's voxel centre, half size h
DXV_HD bool surface_overlap(const float a[3], const float b[3], const float d[3], float cx, float cy, float cz, float h)
{
    const float v0x = a[0] - cx, v0y = a[1] - cy, v0z = a[2] - cz;
    const float v1x = b[0] - cx, v1y = b[1] - cy, v1z = b[2] - cz;
    const float v2x = d[0] - cx, v2y = d[1] - cy, v2z = d[2] - cz;
    // the box's face normals
    if (min3_(v0x, v1x, v2x) > h || max3_(v0x, v1x, v2x) < -h) return false;
    if (min3_(v0y, v1y, v2y) > h || max3_(v0y, v1y, v2y) < -h) return false;
    if (min3_(v0z, v1z, v2z) > h || max3_(v0z, v1z, v2z) < -h) return false;
    // the nine edge cross products
    const float e0x = v1x - v0x, e0y = v1y - v0y, e0z = v1z - v0z;
    const float e1x = v2x - v1x, e1y = v2y - v1y, e1z = v2z - v1z;
    const float e2x = v0x - v2x, e2y = v0y - v2y, e2z = v0z - v2z;
    const float ex[3] = {e0x, e1x, e2x}, ey[3] = {e0y, e1y, e2y}, ez[3] = {e0z, e1z, e2z};
#pragma unroll
    for (int e = 0; e < 3; ++e) {
        if (surface_edge_separates(ey[e], ez[e], v0y, v0z, v1y, v1z, v2y, v2z, h)) return false;     // i = x: (j, k) = (y, z)
        if (surface_edge_separates(ez[e], ex[e], v0z, v0x, v1z, v1x, v2z, v2x, h)) return false;     // i = y: (j, k) = (z, x)
        if (surface_edge_separates(ex[e], ey[e], v0x, v0y, v1x, v1y, v2x, v2y, h)) return false;     // i = z: (j, k) = (x, y)
    }
    // the triangle's plane
    const float nx = e0y * e1z - e0z * e1y, ny = e0z * e1x - e0x * e1z, nz = e0x * e1y - e0y * e1x;
    const float vminx = (nx > 0.0f ? -h : h) - v0x, vmaxx = (nx > 0.0f ? h : -h) - v0x;
    const float vminy = (ny > 0.0f ? -h : h) - v0y, vmaxy = (ny > 0.0f ? h : -h) - v0y;
    const float vminz = (nz > 0.0f ? -h : h) - v0z, vmaxz = (nz > 0.0f ? h : -h) - v0z;
    if ((nx * vminx + ny * vminy) + nz * vminz > 0.0f) return false;
    if (!((nx * vmaxx + ny * vmaxy) + nz * vmaxz >= 0.0f)) return false;
    return true;
}

// Candidate voxels of a triangle: its box in voxel units (x, z: (p + 1) N / 2; y flipped: (1 - p) N / 2, voxel i spans [i, i + 1]),
// widened by 1/16 voxel and clipped to the grid.  Returns false when nothing is left (or a vertex is not finite).
// Why 1/16 is enough, for vertices of any size (a refitted mesh can leave the bound of its build): a voxel the test accepts passes the
// face test of every axis k, fl(m - c) <= h with m the smallest vertex coordinate (min3 of rounded differences = the rounded
// difference of the minimum: rounding is monotone).  Rounding to nearest then gives m - c <= h (1 + 2^-24) whatever the size of m or
// of the other vertices, so only m itself enters, and only when it lies within a voxel of the grid (|m| <= 1 + 2 h; farther out the
// clip to the grid decides).  c and h are within an ulp of the exact centre and half size, (m + 1) N / 2 within an ulp of 2 scaled
// by N / 2: all together under 10^-3 voxel at N = 2048 (the same for the largest coordinate; tests/test_surface_rule.py checks the
// box against the restated test on triangles with vertices up to 10^6 outside the grid).
DXV_HD bool surface_box(const float a[3], const float b[3], const float d[3], uint32_t N, int lo[3], int hi[3])
{
    const float half = 0.5f * (float)N, m = 0.0625f;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const float mn = min3_(a[k], b[k], d[k]), mx = max3_(a[k], b[k], d[k]);
        if (!(mn == mn && mx == mx && abs_(mn) < 1e30f && abs_(mx) < 1e30f)) return false;
        float u0 = k == 1 ? (1.0f - mx) * half : (mn + 1.0f) * half;
        float u1 = k == 1 ? (1.0f - mn) * half : (mx + 1.0f) * half;
        u0 = min_(max_(__builtin_floorf(u0 - m), -1.0f), (float)N);       // (clamped before any conversion to int)
        u1 = min_(max_(__builtin_floorf(u1 + m), -1.0f), (float)N);
        lo[k] = u0 < 0.0f ? 0 : (int)u0;
        hi[k] = u1 > (float)(N - 1u) ? (int)N - 1 : (int)u1;
        if (lo[k] > hi[k]) return false;
    }
    return true;
}

// ---- the candidate enumeration of csrc/surface.hip's two kernels, host-callable so that tests/hostcheck/surface_check.cpp runs the
// ---- very same code on the CPU -----------------------------------------------------------------------------------------------------------
constexpr uint32_t kSurfaceSmall = 64;        // candidate voxels a lane tests on its own

struct SurfaceGrid {
    uint8_t* grid;
    uint32_t N, z0, nz, zBlock, zPeriod, zLast;     // zLast: the partition's last global slice
    float h;                                        // half a voxel, 1.0f / N
    uint32_t items;                                 // work items the list may take (kSurfaceItems; fewer under option surfaceitems)
};

struct SurfaceTri { float a[3], b[3], d[3]; };

// the candidate box, its z range clipped to the partition's first and last slice
DXV_HD bool tri_box(const SurfaceGrid& g, const SurfaceTri& t, int lo[3], int hi[3])
{
    if (!surface_box(t.a, t.b, t.d, g.N, lo, hi)) return false;
    lo[2] = lo[2] > (int)g.z0 ? lo[2] : (int)g.z0;
    hi[2] = hi[2] < (int)g.zLast ? hi[2] : (int)g.zLast;
    return lo[2] <= hi[2];
}

// global slice z (z0 <= z <= zLast) -> local slice of the partition, or false when the partition does not hold it
DXV_HD bool local_slice(const SurfaceGrid& g, int z, uint32_t& lz)
{
    const uint32_t dz = (uint32_t)z - g.z0, q = dz / g.zPeriod, r = dz - q * g.zPeriod;
    lz = q * g.zBlock + r;
    return r < g.zBlock && lz < g.nz;
}

// a box its triangle's own lane tests voxel by voxel (the count in 64 bits: a box can hold 2048^3 voxels)
DXV_HD bool box_is_small(const int lo[3], const int hi[3])
{
    const uint32_t nx = (uint32_t)(hi[0] - lo[0] + 1), ny = (uint32_t)(hi[1] - lo[1] + 1), nz = (uint32_t)(hi[2] - lo[2] + 1);
    return (uint64_t)nx * ny * nz <= kSurfaceSmall;
}

// What the column walk below may assume of the float32 test, and where it stops assuming it.  The walk follows the EXACT triangle
// (double precision): a column is dropped when its square, widened by half a voxel, misses the exact projection, and a kept column
// tests the depths within one voxel of the exact plane.  That is a superset only while the float32 test accepts no voxel whose box
// is farther than that from the exact triangle.  How far it can be, with u = 2^-24, R = the largest |coordinate| of the triangle
// plus 1 (the centre's) and everything in normalised units:
//   - a vertex enters as fl(p - c): moved by at most u R, differently for every voxel;
//   - an edge component fl(v_b - v_a) is off the exact one by at most 4 u R (two vertices, one rounding of up to 2 R);
//   - an axis test compares p_m = fl(fl(e_j v_mk) - fl(e_k v_mj)) with r = fl(fl(|e_j| h) + fl(|e_k| h)).  With s = |e_j| + |e_k|,
//     p_m / s is the exact projection of v_m onto the axis scaled to unit 1-norm, off by at most 2 u R (each product by u times
//     itself, the difference by u times at most their sum), and r / s = h (1 +- 3 u): the test is the exact one of the rounded
//     triangle against a box of half size h + 2 u R, along the axis the rounded edge gives.  The plane test is the same with three
//     products (3 u R);
//   - that axis is not the exact edge's.  Both pass within 4 u R of the edge's two (rounded) ends, so between them the two lines
//     are 4 u R apart, and beyond an end they part in proportion: for an edge at least half as long as its ends are far out, a
//     voxel of the grid lies within two edge lengths of an end, 5 x 4 u R.  (A shorter edge with far ends has the grid in its
//     extension only where the other two edges cull already; an edge shorter than its own rounding gives an arbitrary axis,
//     which then culls nothing that the face tests of the two nearly equal vertices do not.)
// Together the float32 test accepts nothing farther than (1 + 2 + 20) u R < 24 u R from the exact triangle: 12 u R N voxels.  With
// R <= 2 max(M, 1), M the largest |coordinate|, that is 24 M N / 2^24 voxels, and half of the half voxel the column cull allows --
// the other half is left to second-order terms and to the plane's tilt, which the depth range's whole voxel covers by the same
// margin (a dominant axis: at most sqrt 3 of depth per unit of distance) -- is kept while  M N <= 2^24 / 96, rounded down to
//     kSurfaceFar = 2^17:   N = 64: M <= 2048,   N = 2048: M <= 64.
// A triangle beyond it (a refitted mesh keeps the bound of its build: a vertex can be anywhere) walks EVERY column of its box over
// its whole depth range: the float32 test alone decides, whatever its noise, as it does on the small path -- so a partition's share
// equals those slices of the whole grid although the z clip changes which path a triangle takes.  A mesh inside its bound
// (M <= 1 + 2 h) is below the limit at every grid side: its candidates, and so its timings, are what they were without the limit.
// (Seen first in a numpy mirror of the walk: at N = 64, with vertices of magnitude 10^4.5 to 10^6, about one triangle in six lost
// voxels, the worst 490 of 2,130; tests/test_surface_walk.py holds both enumerations to the test applied to the whole box.)
constexpr float kSurfaceFar = 131072.0f;

// Column set-up of the large path, in voxel units and double precision (the triangle's plane decides which depths a column tests;
// a plane made of rounded float products could be far off for a sliver), with the axes renamed: w = the normal's dominant axis,
// (u, v) = (w + 1, w + 2) mod 3 the plane the triangle is projected onto.
struct SurfaceCols {
    double au, av, aw, bu, bv, du, dv;   // the vertices' (u, v) and a's depth
    double nu, nv, nw;                   // the normal
    int w, u0, v0, w0, w1, rowCols;      // box: columns from (u0, v0), rowCols of them per row, depths [w0, w1]
    uint32_t cols;
    bool plane;                          // false: (nearly) degenerate, or far -- every column tests its whole depth range in the box
    bool cull;                           // false: far -- no column is dropped
};

DXV_HD double vox(float p, int k, double half) { return k == 1 ? (1.0 - (double)p) * half : ((double)p + 1.0) * half; }

// wholeBoxWhenFar = false is the enumeration without the limit above: for tests/hostcheck only, which shows what it loses
DXV_HD void cols_setup(const SurfaceGrid& g, const SurfaceTri& t, const int lo[3], const int hi[3], SurfaceCols& s, bool wholeBoxWhenFar = true)
{
    const double half = 0.5 * (double)g.N;
    const double A[3] = {vox(t.a[0], 0, half), vox(t.a[1], 1, half), vox(t.a[2], 2, half)};
    const double B[3] = {vox(t.b[0], 0, half), vox(t.b[1], 1, half), vox(t.b[2], 2, half)};
    const double D[3] = {vox(t.d[0], 0, half), vox(t.d[1], 1, half), vox(t.d[2], 2, half)};
    const double e1x = B[0] - A[0], e1y = B[1] - A[1], e1z = B[2] - A[2];
    const double e2x = D[0] - A[0], e2y = D[1] - A[1], e2z = D[2] - A[2];
    const double nx = e1y * e2z - e1z * e2y, ny = e1z * e2x - e1x * e2z, nz = e1x * e2y - e1y * e2x;
    const double ax = __builtin_fabs(nx), ay = __builtin_fabs(ny), az = __builtin_fabs(nz);
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
    const double l1 = __builtin_fmax(__builtin_fabs(e1x), __builtin_fmax(__builtin_fabs(e1y), __builtin_fabs(e1z)));
    const double l2 = __builtin_fmax(__builtin_fabs(e2x), __builtin_fmax(__builtin_fabs(e2y), __builtin_fabs(e2z)));
    const float m = max_(max3_(max3_(abs_(t.a[0]), abs_(t.a[1]), abs_(t.a[2])), max3_(abs_(t.b[0]), abs_(t.b[1]), abs_(t.b[2])), abs_(t.d[0])),
                         max_(abs_(t.d[1]), abs_(t.d[2])));
    const bool isFar = wholeBoxWhenFar && m * (float)g.N > kSurfaceFar;
    s.cull = !isFar;
    s.plane = !isFar && __builtin_fabs(s.nw) > 1e-9 * l1 * l2;
    s.rowCols = u1 - u0 + 1;
    s.cols = (uint32_t)s.rowCols * (uint32_t)(v1 - v0 + 1);
}

// one edge of the projected triangle against a column's square of half size 1 (the column's own square widened by half a voxel)
DXV_HD bool edge2_separates(double pu, double pv, double qu, double qv, const SurfaceCols& s, double cu, double cv)
{
    const double gu = pv - qv, gv = qu - pu;
    const double pa = gu * s.au + gv * s.av, pb = gu * s.bu + gv * s.bv, pd = gu * s.du + gv * s.dv;
    const double c = gu * cu + gv * cv, r = __builtin_fabs(gu) + __builtin_fabs(gv);
    return __builtin_fmin(pa, __builtin_fmin(pb, pd)) > c + r || __builtin_fmax(pa, __builtin_fmax(pb, pd)) < c - r;
}

// column `col` of the box's (u, v) rectangle, at (iu, iv): false when it is skipped (its widened square misses the projected triangle);
// else [k0, k1], the depths the plane reaches over the square, one voxel more on either side, clipped to the box
DXV_HD bool column_range(const SurfaceCols& s, uint32_t col, int& iu, int& iv, int& k0, int& k1)
{
    iu = s.u0 + (int)(col % (uint32_t)s.rowCols);
    iv = s.v0 + (int)(col / (uint32_t)s.rowCols);
    const double cu = (double)iu + 0.5, cv = (double)iv + 0.5;
    if (s.cull && (edge2_separates(s.au, s.av, s.bu, s.bv, s, cu, cv) || edge2_separates(s.bu, s.bv, s.du, s.dv, s, cu, cv) ||
                   edge2_separates(s.du, s.dv, s.au, s.av, s, cu, cv)))
        return false;
    k0 = s.w0;
    k1 = s.w1;
    if (s.plane) {
        const double wc = s.aw - (s.nu * (cu - s.au) + s.nv * (cv - s.av)) / s.nw;
        const double sp = 0.5 * (__builtin_fabs(s.nu) + __builtin_fabs(s.nv)) / __builtin_fabs(s.nw);
        // (clamped into [w0 - 1, w1 + 1] before the conversion; a NaN leaves the whole range)
        k0 = (int)__builtin_fmin(__builtin_fmax(__builtin_floor(wc - sp) - 1.0, (double)s.w0), (double)s.w1 + 1.0);
        k1 = (int)__builtin_fmax(__builtin_fmin(__builtin_floor(wc + sp) + 1.0, (double)s.w1), (double)s.w0 - 1.0);
    }
    return true;
}

// the voxel (x, y, z) of depth k in column (iu, iv)
DXV_HD void column_voxel(const SurfaceCols& s, int iu, int iv, int k, int& x, int& y, int& z)
{
    x = s.w == 0 ? k : (s.w == 1 ? iv : iu);
    y = s.w == 0 ? iu : (s.w == 1 ? k : iv);
    z = s.w == 0 ? iv : (s.w == 1 ? iu : k);
}

}  // namespace dxv
