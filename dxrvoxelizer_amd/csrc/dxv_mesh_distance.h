// dxv_mesh_distance.h -- the exact distance from a voxel centre to the mesh (d2(p) = min over triangles of f(p; a, b, c)).
// f is the smallest of four squared distances from p to a COMPUTED POINT of the triangle -- the nearest point of each edge, and the foot
// of the perpendicular where it lies inside -- float32 in a fixed order, so that a minimum over the triangles does not depend on the
// order they are visited in: the LBVH walk, the brute-force kernel, the CPU build of this text and the numpy restatement give the same bits.
// Everything here is __host__ __device__: mesh_distance.hip runs it on the GPU, tests/test_mesh_distance_rule.py compiles it for the CPU.
//
// The cull rule (the one place where the hierarchy could change a result).  A subtree is skipped only when
//     lb(p, box) > best * kMdCullRel + cullAbs,     cullAbs = kMdCullAbs * M^2,     M = max(1, largest |coordinate| of the root box)
// with lb the float32 squared distance from p to the subtree's box (a superset of every member triangle) and best the smallest f so far.
// Why that is enough, u = 2^-24, every coordinate and p within [-M, M]:
//   * a term of f is |p - q|^2 for a computed point q.  q differs from an exact point X of the triangle by at most 18 u M per component
//     (the rounded edge vectors 2 u M each, the rounded products 2 u M each, the two sums 3 u M and 5 u M, v + w <= 1 holding only after
//     rounding 2 u M): |q - X| <= 18 sqrt(3) u M < E = 2^-19 M.  The difference and the dot product add a relative 6 u to the square, so
//     sqrt(f) >= (D - E) (1 - 3 u) for the true distance D to the triangle, and D >= LB, the true distance to the box;
//   * lb rounds five times per term: sqrt(lb) <= LB (1 + 3 u).
//   So f > best is certain once sqrt(lb) > sqrt(best) (1 + 7 u) + E (1 + 6 u).  Squared, with 2 s E <= s^2 2^-10 + E^2 2^10:
//     lb > best (1 + 2^-10 + 2^-19) + E^2 (2^10 + 2)  is implied by  lb > best (1 + 2^-9) + 2^-26 M^2
//   -- which leaves a factor of two on the absolute term and 2^-10 on the relative one for the rounding of the right-hand side itself.
// The comparison is strict and the margin positive: a triangle with f == best is always visited, so tri(p) -- the smallest caller's index
// among the minimisers, compared only on equal f -- is exact too.  The margin costs visits (0.1 % of the distance, 1.2e-4 M in absolute
// terms next to the surface), never results.
#pragma once
#include <math.h>
#include "dxv_types.h"

#pragma clang fp contract(off)

namespace dxv {

constexpr uint32_t kMdNoTriangle = 0xffffffffu;      // tri(p) where the band's cap is strictly smaller than every f
constexpr uint32_t kMdMaxBand = 4096u;
constexpr float kMdCullRel = 1.001953125f;           // 1 + 2^-9
constexpr float kMdCullAbs = 1.4901161193847656e-08f; // 2^-26 (times M^2)

DXV_HD float md_min(float a, float b) { return __builtin_fminf(a, b); }
DXV_HD float md_max(float a, float b) { return __builtin_fmaxf(a, b); }
DXV_HD float md_dot(float ux, float uy, float uz, float vx, float vy, float vz) { return (ux * vx + uy * vy) + uz * vz; }

// squared distance from p to the nearest computed point of the segment a b (a zero-length edge: to a)
DXV_HD float md_seg(float px, float py, float pz, float ax, float ay, float az, float bx, float by, float bz)
{
    const float ex = bx - ax, ey = by - ay, ez = bz - az;
    const float wx = px - ax, wy = py - ay, wz = pz - az;
    const float ee = md_dot(ex, ey, ez, ex, ey, ez);
    float t = ee > 0.0f ? md_dot(wx, wy, wz, ex, ey, ez) / ee : 0.0f;
    t = md_min(md_max(t, 0.0f), 1.0f);
    const float tx = t * ex, ty = t * ey, tz = t * ez;
    const float dx = px - (ax + tx), dy = py - (ay + ty), dz = pz - (az + tz);
    return md_dot(dx, dy, dz, dx, dy, dz);
}

// ... to the foot of the perpendicular on the triangle's plane where it lies inside the triangle; +inf where it does not, or there is no plane
DXV_HD float md_face(float px, float py, float pz, float ax, float ay, float az, float bx, float by, float bz, float cx, float cy, float cz)
{
    const float abx = bx - ax, aby = by - ay, abz = bz - az;
    const float acx = cx - ax, acy = cy - ay, acz = cz - az;
    const float apx = px - ax, apy = py - ay, apz = pz - az;
    const float d00 = md_dot(abx, aby, abz, abx, aby, abz), d01 = md_dot(abx, aby, abz, acx, acy, acz), d11 = md_dot(acx, acy, acz, acx, acy, acz);
    const float d20 = md_dot(apx, apy, apz, abx, aby, abz), d21 = md_dot(apx, apy, apz, acx, acy, acz);
    const float t0 = d00 * d11, t1 = d01 * d01;
    const float den = t0 - t1;
    const float v0 = d11 * d20, v1 = d01 * d21, w0 = d00 * d21, w1 = d01 * d20;
    const float safe = den > 0.0f ? den : 1.0f;
    const float v = (v0 - v1) / safe, w = (w0 - w1) / safe;
    const float s = v + w;
    const bool valid = den > 0.0f && v >= 0.0f && w >= 0.0f && s <= 1.0f;
    const float vx = v * abx, vy = v * aby, vz = v * abz;
    const float ux = w * acx, uy = w * acy, uz = w * acz;
    const float dx = px - ((ax + vx) + ux), dy = py - ((ay + vy) + uy), dz = pz - ((az + vz) + uz);
    const float r = md_dot(dx, dy, dz, dx, dy, dz);
    return valid ? r : __builtin_inff();
}

// f(p; a, b, c)
DXV_HD float md_tri(float px, float py, float pz, const F4& a, const F4& b, const F4& c)
{
    const float s0 = md_seg(px, py, pz, a.x, a.y, a.z, b.x, b.y, b.z);
    const float s1 = md_seg(px, py, pz, b.x, b.y, b.z, c.x, c.y, c.z);
    const float s2 = md_seg(px, py, pz, c.x, c.y, c.z, a.x, a.y, a.z);
    return md_min(md_min(md_min(s0, s1), s2), md_face(px, py, pz, a.x, a.y, a.z, b.x, b.y, b.z, c.x, c.y, c.z));
}

// the caller's triangle index of a record (raw bits of v0.w)
DXV_HD uint32_t md_index(const TriPos& t)
{
    uint32_t i;
    __builtin_memcpy(&i, &t.v0.w, 4);
    return i;
}

// the minimum so far and its smallest index
struct MdBest {
    float d2;
    uint32_t tri;
};
DXV_HD void md_take(MdBest& b, float f, uint32_t index)
{
    const bool better = f < b.d2 || (f == b.d2 && index < b.tri);
    b.d2 = better ? f : b.d2;
    b.tri = better ? index : b.tri;
}
DXV_HD void md_take(MdBest& b, float px, float py, float pz, const TriPos& t) { md_take(b, md_tri(px, py, pz, t.v0, t.v1, t.v2), md_index(t)); }

// what the minimum starts from: +inf, or with a band of B voxels (R * R), R = B * h, h = 2 / N
DXV_HD float md_cap(uint32_t N, uint32_t band)
{
    if (!band) return __builtin_inff();
    const float h = 2.0f / (float)N;
    const float R = (float)band * h;
    return R * R;
}

// squared distance from p to a box, 0 inside
DXV_HD float md_box_lb(float px, float py, float pz, float lox, float loy, float loz, float hix, float hiy, float hiz)
{
    const float dx = md_max(md_max(lox - px, 0.0f), px - hix);
    const float dy = md_max(md_max(loy - py, 0.0f), py - hiy);
    const float dz = md_max(md_max(loz - pz, 0.0f), pz - hiz);
    return md_dot(dx, dy, dz, dx, dy, dz);
}
// true: no triangle inside the box can reach `best` (rel, abs: kMdCullRel and kMdCullAbs * M^2; anything else only in tests)
DXV_HD bool md_cull(float lb, float best, float rel, float abs) { return lb > best * rel + abs; }
// cullAbs for a scene whose root box is [lo, hi]
DXV_HD float md_cull_abs(const float lo[3], const float hi[3])
{
    float m = 1.0f;
    for (int a = 0; a < 3; ++a) m = md_max(m, md_max(__builtin_fabsf(lo[a]), __builtin_fabsf(hi[a])));
    return kMdCullAbs * (m * m);
}

// the field's element: format 0 = voxel units (like dxv_distance), 1 = normalised units; negative where the grid's byte is non-zero
DXV_HD float md_value(float d2, bool solid, int format, uint32_t N)
{
    const float d = sqrtf(d2);
    const float v = format == 0 ? d * (0.5f * (float)N) : d;
    return solid ? -v : v;
}

// The walk over the two-box nodes, one query point: what the kernel does per wave, here per point (the CPU build's cross-check of the
// cull rule; `stack` holds kMdStack entries, enough for any tree of that height: one pending sibling per level).
constexpr int kMdStack = 64;
DXV_HD void md_walk(MdBest& best, float px, float py, float pz, const Node* nodes, const TriPos* tris, int32_t* stack, float rel, float abs)
{
    int sp = 0;
    int32_t node = 0;
    for (;;) {
        const Node& n = nodes[node];
        const float lb0 = md_box_lb(px, py, pz, n.lo0x, n.lo0y, n.lo0z, n.hi0x, n.hi0y, n.hi0z);
        const float lb1 = md_box_lb(px, py, pz, n.lo1x, n.lo1y, n.lo1z, n.hi1x, n.hi1y, n.hi1z);
        const bool near0 = lb0 <= lb1;
        const int32_t cA = near0 ? n.c0 : n.c1, cB = near0 ? n.c1 : n.c0;
        const float lbA = near0 ? lb0 : lb1, lbB = near0 ? lb1 : lb0;
        int32_t next = kNoChild;
        if (!md_cull(lbA, best.d2, rel, abs)) {
            if (cA < 0) md_take(best, px, py, pz, tris[~cA]);
            else next = cA;
        }
        if (!md_cull(lbB, best.d2, rel, abs)) {
            if (cB < 0) md_take(best, px, py, pz, tris[~cB]);
            else if (next == kNoChild) next = cB;
            else stack[sp++] = cB;
        }
        if (next == kNoChild) {
            if (!sp) return;
            next = stack[--sp];
        }
        node = next;
    }
}

} // namespace dxv
