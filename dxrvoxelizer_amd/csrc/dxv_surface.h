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

}  // namespace dxv
