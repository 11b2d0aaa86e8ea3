// dxv_dirmap.h -- direction-space candidate lists for the reference rule (shared by the kernels,
// the device builder and tests/hostcheck).
//
// Every ray of the reference rule is radial: origin p = voxel centre, direction p / |p|
// (Content/Shaders/DXRVoxelizer.hlsl:44-53), so the points of a ray are (rho + t) * dir with
// rho = |p|: in direction space a ray is one POINT plus a start radius.  A cube map around the grid
// centre (6 faces of R x R texels, face coordinates u = p_b / |p_a|, v = p_c / |p_a| on the face of
// the dominant axis a) lists, per texel, the triangles whose projection can reach it.  A ray reads
// the list of its texel and hands the few entries whose footprint box contains (u, v) and whose
// radial range lies beyond rho to the same canonical triangle step as the tree walks
// (leaf_reference: padded-box slab test, watertight test, closest = min (t, k)).  No stack, no tree.
//
// Identical results need only one property: every triangle that leaf_reference would accept for a
// ray is listed in that ray's texel with a footprint containing the ray and a radial range that
// passes.  leaf_reference accepts a triangle when the ray passes the slab test of its box padded by
// 2^-16 AND the fp32 watertight test (tri_test, dxv_math.h).
//
// THE WIDE PAD.  For a degenerate sliver, whose edge functions all vanish along its line, only the padded
// box keeps the ray within sqrt(3) 2^-16 = 2.64e-5 of it: footprints are those of the triangle dilated by
// kDmDelta = 2^-15 = 3.05e-5 (in face coordinates 2.25 delta / dmin, dm_footprint_finish), clipped against
// face frusta widened by 2^-10, and then rounded outward to halfs; triangles closer than 64 kDmDelta to
// the centre along the face axis take the whole face.  Radial margins (+-4 delta), `thick`, the 64 delta
// rule and the frustum planes are all made with this delta, for every triangle.
//
// THE TRIANGLE'S OWN LATERAL BOUND (dm_lateral_pad; option lateralpad).  A whole projected triangle that is
// not degenerate is held by the watertight test itself, far closer than by its box; sideways -- and only
// sideways -- its record is dilated by the smaller of the wide pad and the bound below.  u = 2^-24: a rounded
// fp32 result r is within u |r| of the exact one.  All coordinates lie in [-1, 1].
//  1  Sheared coordinates.  tri_test computes A = fl(v - o) per axis (|v - o| <= 2: off by <= 2 u each) and
//     Ax = fma(-Sx, akz, akx) with |Sx| <= 1, |Ax| <= 4: one rounding, <= 4 u, plus the two inherited ones,
//     2 u + 2 u.  Every sheared coordinate is within E = 8 u of the exact projection of v - o along the
//     line L' through o with direction D = (Sx, Sy, 1) (in the ray's kx, ky, kz).
//  2  Size.  An accepted ray has passed the slab test of the padded box; taken as 2^-15 per axis that also
//     pays for the slab's own roundings (its t values are <= 3.5 where it decides, off by a few u) and for
//     the slab's line against L'.  So some point of L' lies within diag + 2 sqrt(3) 2^-15 of every vertex
//     (diag: the diagonal of the triangle's box), and the projection along D stretches by at most
//     sqrt(1 + Sx^2 + Sy^2) <= sqrt(3): every sheared vertex lies within Dm = sqrt(3) (diag + 2 sqrt(3) 2^-15)
//     of the ray.
//  3  Edge functions.  U = fl(fl(Cx By) - fl(Cy Bx)) (no contraction).  Against the exact U^ of the exact
//     sheared vertices: the coordinates' E through the products, E (|B|_1 + |C|_1) + 2 E^2 <= 2 sqrt(2) E Dm
//     + 2 E^2; the three roundings, u (|Cx By| + |Cy Bx|) + u |U| <= 2.01 u Dm^2.  An exact zero is evaluated
//     again in double: exact products, an exact sign -- inside the same bound.
//  4  The line.  L' is not the radial line: Sx = fl(fl(ox / len) / fl(oz / len)), three roundings of which
//     `len`'s own cancel, is within 3.01 u of ox / oz, so D = D0 + dD with D0 = o / o_kz and |dD| <= 4.26 u.
//     U^ is the triple product [D, C - o, B - o]; the share of dD is at most |dD| |C - o| |B - C| <=
//     4.26 u * 2 sqrt(3) * diag <= 15 u diag.  In all a computed edge function is within
//         e1 = 2 sqrt(2) E Dm + 2 E^2 + 2.01 u Dm^2 + 15 u diag
//     of [D0, C - o, B - o] = [D0, C, B] (o is parallel to D0), the edge function of the TRUE radial line.
//  5  Face coordinates.  With o = |o_a| (u_r, v_r, 1), C = d_C (u_C, v_C, 1), B = d_B (u_B, v_B, 1) on the
//     ray's face (a: the face axis, d: depths >= dmin >= 64 delta), [D0, C, B] = +- (|o_a| / |o_kz|) d_C d_B
//     e_CB (u_r, v_r), e_CB the edge function of the PROJECTED triangle, |o_a| / |o_kz| >= 1 (a is o's
//     largest axis).  tri_test accepts when the three computed signs agree.  All three >= 0 (with the
//     triangle's orientation): every e_k (u_r, v_r) >= -e1', e1' = e1 / dmin^2.  All three <= 0: every e_k
//     <= e1', but the three sum to twice the projected area -- impossible once 2 area > 3 e1'.
//  6  Shape.  e_k >= -e1' puts the ray within e1' / l_k of edge k's line (l_k: its projected length), and
//     inside the triangle of the three lines so moved, whose corner at the vertex between edges a and b
//     lies at most (e1' / l_a + e1' / l_b) / sin(angle) = e1' (l_a + l_b) / (2 area) <= 2 e1' / hmin from it,
//     hmin = 2 area / l_max the projected triangle's smallest altitude (no edge is shorter than hmin).  So
//         pad = 2 e1 / (dmin^2 hmin)
//     holds the ray inside every edge pushed out by pad AND inside the box of the projected vertices widened
//     by pad: what dm_rect, dm_texel_test and dm_local_entry ask.  Beyond the end of a short edge the second
//     edge function is definitely negative from this distance on.  Shape enters through the PROJECTED
//     triangle: a well-shaped triangle seen at a grazing angle has a small hmin and gets a large pad or none.
//     The bound is used where pad < hmin / 2 (then e1' < hmin^2 / 4 <= area / 2: step 5's second case is
//     excluded).
//  7  The other roundings, as before: + 1e-6 for the ray's own dm_ray_point / dm_local (u and the cell are
//     within 2 u of exact), + 1e-6 for the record's fp32 vertices; dm_lateral_pad's own double arithmetic
//     takes 1 %.
// The wide pad stays, explicitly, for records without a projected triangle (hasTri 0: a vertex within
// 64 delta of the face plane), clipped polygons, a box cut to the face, coordinates beyond the unit cube,
// projections (nearly) edge-on (twice the area <= 1e-3 of the squared edges: the threshold of dm_texel_test
// and dm_local_radial) and altitudes below 2 pad.  At the headline's scale (triangles of 0.008 at depth 0.6
// on the 512 map) the lateral band falls from 3.8 cells of a texel's 128 to about 0.5.
// tests/test_lateral_pad.py casts millions of rays at and around every edge of seeded families of
// triangles through this very code and finds every accepted ray listed -- and with the pad at zero does not.
#pragma once
#include "dxv_trace.h"

namespace dxv {

// One entry per (triangle, texel), everything in small integers so that a ray decides in a handful of integer
// instructions whether the triangle is worth the 48-byte fetch and the watertight test:
//   box   bytes (x0, y0, 127 - x1, 127 - y1): the footprint's box, cut to the texel, in texel-local cells (a texel is
//         128 x 128 cells).  A ray in cell (x, y) passes iff every byte of (x, y, 127 - x, 127 - y) is >= this word's
//         byte: one subtraction of packed bytes (dm_local_pass).
//   edge  signed bytes (a, b, c1, c2): the ONE edge of the projected, dilated triangle that cuts most off that box.
//         The ray passes iff a (x - 64) + b (y - 64) + 127 c1 + c2 >= 0 (one v_dot4c_i32_i8; cells from the texel's
//         centre, so that every line through the texel has a constant the two bytes hold: dm_local_entry); 0 = no edge
//         (clipped polygons, or no edge crosses the box).  A triangle fills at most half of its box: this halves the
//         triangle tests.
//   rr    (0x7fff - r0) | r1 << 16 | 0x80008000, r0 / r1 the outward-rounded radial range as halfs: positive halfs
//         order like integers, so r1 >= near and r0 <= (start + closest hit) are one packed subtraction as well.
//   tri   position in the scene's triangle order (TriPos index) in the low 26 bits; the high 6 bits say how far behind this
//         entry's far radius the EARLIEST start of any later entry of the texel lies, in 63rds of the texel's thickest
//         entry (rounded up): the scan stops at the first entry for which that point is beyond the closest hit
//         (dm_stop_radius).  Lists therefore serve scenes of up to 2^26 triangles.
struct alignas(16) DirEntry {
    uint32_t box, edge, rr, tri;
};
static_assert(sizeof(DirEntry) == 16, "one 16-byte load per entry");
constexpr uint32_t kDmCells = 128u;                 // cells per texel side (7 bits)

// Record of a (triangle, face) pair, builder side: the footprint as before plus the projected triangle, from which
// the per-texel entries are cut.
struct alignas(16) DirRecord {
    float u0, u1, v0, v1;      // footprint box in face coordinates, rounded outward; u0 > u1: no footprint
    uint32_t rr;               // radial range of the whole footprint, halfs rounded outward: r0 | r1 << 16
    uint32_t hasTri;           // bit 0: px / py / pw hold the projected triangle (all three vertices in front of the face plane); bit 1: dm_record_on_map;
                               // bit 2 (kDmRecLateral): made with the per-record lateral bound, bits 3 .. 31 = the low 29 bits of the 2^-15 pad (dm_wide_pad)
    float pad;                 // dilation of the projected triangle in face coordinates: the smaller of the 2^-15 pad and the triangle's own bound (dm_lateral_pad)
    float px[3], py[3];        // projected vertices
    float pw[3];               // 1 / depth of the vertices along the face axis: linear over the projected triangle's plane (dm_local_radial)
};
static_assert(sizeof(DirRecord) == 64, "record layout");
constexpr uint32_t kDmRecLateral = 4u;
struct DirBox { float u0, u1, v0, v1; };
// the 2^-15 pad of a record (what `pad` was before triangles had a bound of their own): which EDGE an entry stores is still chosen
// with it, so that an entry made with the smaller pad stores the same edge with a smaller constant -- its cells a subset
DXV_HD float dm_wide_pad(const DirRecord& r) { return (r.hasTri & kDmRecLateral) ? __builtin_bit_cast(float, 0x20000000u | (r.hasTri >> 3)) : r.pad; }
// the footprint box of a record: u0 .. v1 are the box of the 2^-15 pad; a record with a bound of its own takes back 99 % of the
// difference on every side (the last per cent: this subtraction's and the two pads' own rounding, 1e-7 against the 1e-6 both pads carry)
DXV_HD DirBox dm_record_box(const DirRecord& r)
{
    DirBox b{r.u0, r.u1, r.v0, r.v1};
    if (r.hasTri & kDmRecLateral) {
        const float s = 0.99f * (dm_wide_pad(r) - r.pad);
        b.u0 += s; b.u1 -= s; b.v0 += s; b.v1 -= s;
    }
    return b;
}

struct alignas(16) DirCell {                        // one 16-byte load per ray
    uint32_t begin;                                 // the texel's entries: [begin, begin + count)
    uint16_t count;                                 // (a scene with more than 65,535 entries in one texel keeps the tree walk)
    uint16_t r1max;                                 // far radius of its last entry (half bits): a ray that starts beyond it has no candidate
    uint16_t thick;                                 // largest radial extent r1 - r0 of its entries (half bits, rounded up): the unit of the entries' stop codes
    // The first two steps of the binary search for a ray's start need no load: the far radii (half bits) of the entries
    // the search would look at -- the middle one, and the middles of both halves (dm_search_hints).  Lists of up to 35
    // entries (all of a surface mesh's) are then down to the eight entries a scan round starts with anyway.
    uint16_t q1, q2, q3;
};
static_assert(sizeof(DirCell) == 16, "one 16-byte load per texel");

// entries the start search looks at first in a list of n entries (relative indices; n > 8): the middle of [0, n), and the
// middles of [0, m2) and [m2 + 1, n) where those halves are still longer than 8 -- exactly the sequence of the loop
// `while (hi - lo > 8) { mid = lo + (hi - lo) / 2; r1[mid] < near ? lo = mid + 1 : hi = mid; }`
struct DirSearchHints { uint32_t m1, m2, m3; bool has1, has3; };
DXV_HD DirSearchHints dm_search_hints(uint32_t n)
{
    DirSearchHints h;
    h.m2 = n >> 1;
    h.has1 = h.m2 > 8u;                       // left half [0, m2)
    h.m1 = h.m2 >> 1;
    h.has3 = n - (h.m2 + 1u) > 8u;            // right half [m2 + 1, n)
    h.m3 = h.m2 + 1u + ((n - (h.m2 + 1u)) >> 1);
    return h;
}

struct DirMapView {
    const DirCell* cells;      // 6 * R * R, cell = (face * R + j) * R + i; NULL: no map
    const DirEntry* entries;
    uint32_t R;                // texels per face side, a power of two
    uint32_t coop = 0u;        // device: 1 = a lone lane's long list is scanned by its whole wave (trace_reference_dm_from)
    const uint32_t* starts = nullptr;   // 6 * R * R start words (dm_start_word), indexed like the cells; NULL: every scan begins where the search ends
    const DirCell* startCells = nullptr;    // 6 * R * R start cells (dm_start_cell): a texel's cell with its start word where the hints are; NULL: none
};

constexpr float kDmDelta = 3.0517578125e-5f;        // 2^-15: dilation of the triangles
constexpr double kDmFrustum = 1.0 + 1.0 / 1024.0;   // face frusta are widened by this factor

// texel index of face coordinate u (monotone in u: add, multiply by a power of two, floor)
DXV_HD uint32_t dm_texel(float u, uint32_t R)
{
    const float x = (u + 1.0f) * (0.5f * (float)R);
    if (!(x > 0.0f)) return 0u;
    const uint32_t i = (uint32_t)x;
    return i < R ? i : R - 1u;
}

// texel AND texel-local cell (0 .. 127) of face coordinate u: lexicographically monotone in u, evaluated identically by
// builder and kernel (x - i is exact for x in [i, i + 1), the scaling a power of two)
DXV_HD void dm_local(float u, uint32_t R, uint32_t& texel, uint32_t& cell)
{
    const float x = (u + 1.0f) * (0.5f * (float)R);
    if (!(x > 0.0f)) { texel = 0u; cell = 0u; return; }
    const uint32_t i = (uint32_t)x;
    if (i >= R) { texel = R - 1u; cell = kDmCells - 1u; return; }
    const uint32_t c = (uint32_t)((x - (float)i) * (float)kDmCells);
    texel = i;
    cell = c < kDmCells ? c : kDmCells - 1u;
}

// a . b over four signed bytes (v_dot4c_i32_i8 on the device)
DXV_HD int32_t dm_dot4(uint32_t a, uint32_t b)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_amdgcn_sdot4((int)a, (int)b, 0, false);
#else
    int32_t s = 0;
    for (int k = 0; k < 4; ++k) s += (int32_t)(int8_t)(a >> (8 * k)) * (int32_t)(int8_t)(b >> (8 * k));
    return s;
#endif
}

// The ray's side of an entry test: q = bytes (x, y, 127 - x, 127 - y) | 0x80808080, p = signed bytes (x - 64, y - 64, 127, 1)
// -- the edge word counts cells from the texel's CENTRE --, rc = (0x7fff - half_down(bound)) | half_up(near) << 16 (dm_radial_word)
struct DirRayLocal { uint32_t q, p; };
DXV_HD DirRayLocal dm_ray_local(uint32_t x, uint32_t y)
{
    DirRayLocal l;
    // q in three instructions from w = x | y << 8 where the sum of four shifted bytes took four: the upper bytes (127 - x) | 0x80 =
    // 255 - x = x ^ 0xff are w's complement, shifted.  That pays for the instruction the centred p costs more than the corner's: the
    // kernels' instruction counts stay what they were.  (The empty asm statements pin the three steps: left alone the compiler
    // moves y's shift into the branches y comes out of, builds the complement from x and y again, or adds all three parts at once
    // with the constant in a scalar register -- an instruction more each way.)
#if defined(__HIP_DEVICE_COMPILE__)
    asm("" : "+v"(y));
#endif
    uint32_t w = x | (y << 8);
#if defined(__HIP_DEVICE_COMPILE__)
    asm("" : "+v"(w));
#endif
    uint32_t lo = w + 0x8080u;
#if defined(__HIP_DEVICE_COMPILE__)
    asm("" : "+v"(lo));
#endif
    l.q = ((~w) << 16) + lo;
    // x - 64 in each of the two low bytes: adding 64 cannot carry out of a byte, and flipping bit 7 of the sum is adding 128 more,
    // 192 = -64 in all -- one add and one xor where the corner's word took one or
    l.p = (w + ((127u << 16) | (1u << 24) | 0x4040u)) ^ 0x8080u;
    return l;
}
// Directed float -> half for the values a ray brings to the integer radial test: positive, inside the half's normal
// range [2^-14, 65504) (a ray starts at least half a voxel diagonal, 4e-4 even at 2048^3, from the centre).  There the
// half's bits are the float's, rebiased and cut: truncation rounds down, adding the dropped bits' mask first rounds up
// (the carry runs into the exponent as it should).  Equal to half_down / half_up (dxv_math.h) on that range (tests).
DXV_HD uint32_t dm_half_down_pos(float x) { return (__builtin_bit_cast(uint32_t, x) - 0x38000000u) >> 13; }
DXV_HD uint32_t dm_half_up_pos(float x) { return (__builtin_bit_cast(uint32_t, x) - 0x38000000u + 0x1fffu) >> 13; }
DXV_HD uint32_t dm_radial_word(float near, float bound)
{
    const uint32_t b = bound < 65504.0f ? dm_half_down_pos(bound) : 0x7bffu;
    return (0x7fffu - b) | (dm_half_up_pos(near) << 16);
}
// box, edge and radial range of an entry against a ray: true = fetch and test the triangle
DXV_HD bool dm_local_pass(const DirEntry& e, const DirRayLocal& l, uint32_t rc)
{
    return ((l.q - e.box) & 0x80808080u) == 0x80808080u && ((e.rr - rc) & 0x80008000u) == 0x80008000u && dm_dot4(e.edge, l.p) >= 0;
}
constexpr uint32_t kDmTriBits = 26u, kDmTriMask = (1u << kDmTriBits) - 1u;
DXV_HD uint32_t dm_entry_tri(const DirEntry& e) { return e.tri & kDmTriMask; }
// The lists are sorted by far radius.  No entry from this one on starts before  r1 - q * (thick / 63):  q is chosen by
// the builder (dm_stop_code) with this very expression, so the float arithmetic is the same on both sides.
DXV_HD float dm_stop_step(float thick) { return thick * 0.015873017f; }                     // a little more than 1 / 63
DXV_HD float dm_stop_radius(const DirEntry& e, float step) { return half_bits_to_float((e.rr >> 16) & 0x7fffu) - (float)(e.tri >> kDmTriBits) * step; }
// smallest q in [0, 63] with r1 - q * step <= suffixMinR0 (r1 - 63 * step <= r1 - thick <= every later start: always found)
DXV_HD uint32_t dm_stop_code(float r1, float suffixMinR0, float step)
{
    // start two below the quotient (every smaller q misses by more than a whole step, far beyond rounding) and count up
    const float x = step > 0.0f ? (r1 - suffixMinR0) / step : 0.0f;
    uint32_t q = x > 2.0f ? (x < 65.0f ? (uint32_t)x - 2u : 63u) : 0u;
    while (q < 63u && r1 - (float)q * step > suffixMinR0) ++q;
    return q;
}
DXV_HD float dm_entry_r1(const DirEntry& e) { return half_bits_to_float((e.rr >> 16) & 0x7fffu); }
DXV_HD float dm_entry_r0(const DirEntry& e) { return half_bits_to_float(0x7fffu - (e.rr & 0x7fffu)); }

// face = 2 * axis + (negative side); in-face axes (b, c) = ((axis + 1) % 3, (axis + 2) % 3)
DXV_HD void dm_ray_point(float ox, float oy, float oz, uint32_t& face, float& u, float& v, float& rho)
{
    const float ax = __builtin_fabsf(ox), ay = __builtin_fabsf(oy), az = __builtin_fabsf(oz);
    // (the two quotients share their denominator: div_by, dxv_math.h -- the same bits as `/` for these operands, checked exhaustively)
    float a, nb, nc;
    if (ax >= ay && ax >= az) { face = ox < 0.0f ? 1u : 0u; a = ax; nb = oy; nc = oz; }
    else if (ay >= az) { face = oy < 0.0f ? 3u : 2u; a = ay; nb = oz; nc = ox; }
    else { face = oz < 0.0f ? 5u : 4u; a = az; nb = ox; nc = oy; }
    const RcpRefined byA = rcp_refined(a);
    u = div_by(nb, byA); v = div_by(nc, byA);
    rho = sqrt_in_range((ox * ox + oy * oy) + oz * oz);
}

// ---------------------------------------------------------------------------------------------
// Start table: one 32-bit word per texel, a pure function of the texel's cell and entries (like the max-mip: derived, never
// exported; cells and entries stay as they are).  The start search narrows a list to a window of up to 8 entries and the scan
// begins at the window's left edge: a texel that lists two shells (9 .. 35 entries: only q2 exists up to 17) sends a ray inside
// the body to entry 0 or to n / 2 + 1, and the entries in front of the ray are fetched, four per round, to fail the radial test.
// The word says how many entries a ray may skip, from the ray's start radius alone:
//   key of an entry  ke = the half bits of its far radius r1;  key of a ray  kn = dm_half_down_pos(near);  top = cell.r1max
//   bucket           d(k) = (top - k) >> sh, sh the smallest shift that puts the list's FIRST entry in bucket B - 1 or lower
//   word             sh in bits 0 .. 3; then for d = 0 .. B - 2, in 8 bits each, S[d] = the number of entries with d(ke) > d
//                    in units of ceil(count / 256) entries, rounded down (count <= 65,535: S <= 255)
//   start of a ray   begin + S[d(kn)] * unit, begin itself for d(kn) >= B - 1
// Why a ray loses nothing: d is non-increasing in k, so d(ke) > d(kn) implies ke < kn, i.e. r1 < half(kn) <= near -- the entry fails
// the radial half of dm_local_pass for this ray.  The lists are sorted by r1, so those entries are a prefix of the list; rounding S
// down only skips fewer of them.  The table skips only entries the scan would have looked at and rejected; the stop rule and the
// flush rule do not depend on which entries were looked at before (the cooperative scan relies on the same).  A ray whose key lies
// above `top` (not live) or outside the halfs' range gets no skip at all.
// ---------------------------------------------------------------------------------------------
constexpr uint32_t kDmStartBuckets = 4u;            // B: 4 bits + 3 x 8 bits of the word (the round replay: 8 buckets save 0.02 rounds more)
DXV_HD uint32_t dm_entry_key(const DirEntry& e) { return (e.rr >> 16) & 0x7fffu; }
DXV_HD uint32_t dm_start_unit(uint32_t count) { return (count + 255u) >> 8; }
DXV_HD uint32_t dm_start_bucket(uint32_t top, uint32_t sh, uint32_t k) { return k < top ? (top - k) >> sh : 0u; }
// the word of a texel; list = entries + cell.begin (O(B log count) loads: the buckets' edges by binary search in the sorted list)
DXV_HD uint32_t dm_start_word(const DirCell& cell, const DirEntry* list)
{
    const uint32_t n = cell.count, top = cell.r1max;
    if (n == 0u) return 0u;
    const uint32_t k0 = dm_entry_key(list[0]);
    uint32_t sh = 0u;
    while (dm_start_bucket(top, sh, k0) > kDmStartBuckets - 1u) ++sh;   // (top - k0 < 2^15: sh <= 13)
    const uint32_t unit = dm_start_unit(n);
    uint32_t word = sh;
    for (uint32_t d = 0u; d + 1u < kDmStartBuckets; ++d) {
        uint32_t lo = 0u, hi = n;                                       // first entry with bucket <= d
        while (lo < hi) {
            const uint32_t mid = lo + ((hi - lo) >> 1);
            if (dm_start_bucket(top, sh, dm_entry_key(list[mid])) > d) lo = mid + 1u; else hi = mid;
        }
        word |= (lo / unit) << (4u + 8u * d);                           // (the last entry's key is top, bucket 0: lo <= n - 1, lo / unit <= 255)
    }
    return word;
}
// entries a ray of start radius `near` may skip at the head of the texel's list (word 0: none)
DXV_HD uint32_t dm_start_offset(uint32_t word, uint32_t count, uint32_t top, float near)
{
    const uint32_t kn = dm_half_down_pos(near);
    uint32_t d = kn <= top ? (top - kn) >> (word & 15u) : kDmStartBuckets - 1u;
    if (d > kDmStartBuckets - 1u) d = kDmStartBuckets - 1u;
    return ((word >> (4u + 8u * d)) & 255u) * dm_start_unit(count);     // (d = B - 1 reads the word's four empty top bits: 0)
}
// Start cells: a third array beside cells and table (derived like the table, never exported), a texel's cell with the texel's start word
// where the search hints are -- q1 | q2 << 16 = dm_start_word, q3 = 0; begin, count, r1max and thick byte for byte the canonical cell's, so
// a ray's `live` decision and its stop step come out of either cell alike.  A kernel that reads the table reads THIS cell and nothing else:
// one 16-byte gather per ray instead of a 16-byte and a 4-byte one to the same texel index.  The hints are what it gives up: a list of up to
// kDmStartCellDirect entries begins its scan at the table's start with no search at all, a longer one runs the loaded binary search over
// the whole list (two trips more than behind the hints) and then takes the later of the two starts, as before.  Either way a skipped
// entry has r1 < near (the table's argument above; the search's own invariant): only which rejected entries are looked at changes.
constexpr uint32_t kDmStartCellDirect = 35u;        // (the hints' reach: the lists that take a search load stay the ones that took one)
DXV_HD DirCell dm_start_cell(const DirCell& cell, uint32_t word)
{
    DirCell s = cell;
    s.q1 = (uint16_t)(word & 0xffffu); s.q2 = (uint16_t)(word >> 16); s.q3 = 0u;
    return s;
}
#if defined(DXV_START_WORD_ZERO)                    // (timing-only build: the body that reads start cells with every word 0 -- no skip -- against the _plain body)
DXV_HD uint32_t dm_start_cell_word(const DirCell&)
{
    uint32_t w = 0u;
#if defined(__HIP_DEVICE_COMPILE__)
    asm("" : "+v"(w));                              // (a zero the compiler cannot see: the word's arithmetic stays in the body)
#endif
    return w;
}
#else
DXV_HD uint32_t dm_start_cell_word(const DirCell& startCell) { return (uint32_t)startCell.q1 | ((uint32_t)startCell.q2 << 16); }
#endif
// where the scan of a ray that read a START cell begins (absolute entry index; a ray that is not live: the list's end)
// direct: lists of up to so many entries take no search (kDmStartCellDirect; a parameter for the host's replay); loads: search loads, counted
DXV_HD uint32_t dm_start_cell_begin(const DirCell& sc, const DirEntry* entries, bool live, float near, uint32_t direct = kDmStartCellDirect,
                                    uint32_t* loads = nullptr)
{
    const uint32_t end = sc.begin + sc.count;
    if (!live) return end;
    const uint32_t from = sc.begin + dm_start_offset(dm_start_cell_word(sc), sc.count, sc.r1max, near);
    if (sc.count <= direct) return from;
    uint32_t i = sc.begin, hi = end;
    while (hi - i > 8u) {
        const uint32_t mid = i + ((hi - i) >> 1);
        if (loads) ++*loads;
        if (dm_entry_r1(entries[mid]) < near) i = mid + 1u; else hi = mid;
    }
    return from > i ? from : i;
}

// The first step of a ray through the lists -- its texel, its cell inside the texel, and whether it has any candidate at
// all: a ray whose texel is empty, or that starts beyond the far radius of its texel's last entry, is a miss after this
// one load.  ONE definition: the kernel (trace_reference_dm), the plan's exact checker (k_plan_check, dxv_debug.hip) and
// the exhaustive list check make this decision through it, and the brick test below bounds it from above.
// (startWord: the texel's word of the start table, asked for with the cell -- two independent loads behind one wait; 0 without a table)
// STARTS = false: a kernel compiled for launches WITHOUT a table (startWord is the constant 0 and everything made of it folds away: the
// instruction stream of the kernel before there was a table).  The table's few instructions cost a launch that does not use them 5 - 6 %
// (measured, profiles/start_table/: the body with them, pointer NULL, against the body without), so the brick kernels exist in both forms
// and the launch picks by the pointer (voxelize_lists.hip).
// STARTS = 2: a kernel compiled to read START cells (dm.startCells: the one load; its scan begins by dm_start_cell_begin, startWord stays 0);
// STARTS = 3: start cells where the view has them, else as STARTS = 1 (a wave-uniform choice: the brick-box body, the host).
struct DirRayStart { DirCell cell; uint32_t cx, cy; float rho, near; bool live; uint32_t startWord; };
#if defined(DXV_NO_START_TABLE)
constexpr int dm_starts_form(int) { return 0; }
#else
constexpr int dm_starts_form(int starts) { return starts; }
#endif
template <int FORM> DXV_HD bool dm_reads_start_cells(const DirMapView& dm) { return FORM == 2 || (FORM == 3 && dm.startCells != nullptr); }
template <int STARTS = 1>
DXV_HD DirRayStart dm_ray_start(float ox, float oy, float oz, const DirMapView& dm)
{
    DirRayStart s;
    uint32_t face, ti, tj;
    float u, v;
    dm_ray_point(ox, oy, oz, face, u, v, s.rho);
    dm_local(u, dm.R, ti, s.cx); dm_local(v, dm.R, tj, s.cy);
    const uint32_t at = (face * dm.R + tj) * dm.R + ti;
    constexpr int FORM = dm_starts_form(STARTS);    // (DXV_NO_START_TABLE, an A/B build from the same sources: 0, the kernels as they were without the table)
    s.startWord = 0u;
    if (dm_reads_start_cells<FORM>(dm)) {                               // (wave-uniform)
#if defined(__HIP_DEVICE_COMPILE__)
        // ONE 16-byte load: nothing reads q3 of a start cell, and left to itself the compiler asks for the cell's first twelve bytes and for
        // q2 in two load instructions -- as many as cell and word were.  The empty statement may have changed all four words for all it knows.
        typedef uint32_t Words4 __attribute__((ext_vector_type(4)));
        Words4 w = *reinterpret_cast<const Words4*>(dm.startCells + at);
        asm("" : "+v"(w));
        s.cell = __builtin_bit_cast(DirCell, w);
#else
        s.cell = dm.startCells[at];
#endif
    }
    else {
        // The word is asked for IN FRONT of the cell, under the (wave-uniform) test of the pointer, and nothing looks at it before the cell
        // has been asked for too: both loads are in flight behind one wait, no dependent trip -- and a launch without a table issues no
        // load for it at all (asked for behind the cell, the compiler waits for the cell in front of the branch).
        if (FORM && dm.starts) s.startWord = dm.starts[at];
        s.cell = dm.cells[at];
    }
    s.near = s.rho * 0.999f;
    s.live = s.cell.count != 0u && !(half_bits_to_float(s.cell.r1max) < s.near);
    return s;
}

// ---------------------------------------------------------------------------------------------
// Max-mip of the texels' far radii: which 4 x 4 x 4-voxel bricks can hold a live ray at all (the launch's work queue,
// k_plan_bricks in plan_bricks.hip).  Key of a texel = its r1max as half bits (positive halfs order like integers), 0 for an
// empty texel; level l holds, for 6 faces of (R >> l)^2 cells, the maximum over the 2^l x 2^l texels below a cell.
// Built from the cells (dirmap.hip: dirmap_mip), never exported: a function of the cells alone.
// ---------------------------------------------------------------------------------------------
DXV_HD uint32_t dm_mip_levels(uint32_t R) { uint32_t l = 1u; while ((R >> (l - 1u)) > 1u) ++l; return l; }   // R = 256: 9 (256 .. 1)
DXV_HD uint32_t dm_mip_offset(uint32_t R, uint32_t level)
{
    uint32_t off = 0;
    for (uint32_t l = 0; l < level; ++l) off += 6u * (R >> l) * (R >> l);
    return off;
}
DXV_HD uint32_t dm_mip_words(uint32_t R) { return dm_mip_offset(R, dm_mip_levels(R)); }    // 16-bit words
DXV_HD uint32_t dm_mip_key(const DirCell& c) { return c.count ? (uint32_t)c.r1max : 0u; }
DXV_HD uint32_t dm_mip_count_key(const DirCell& c) { return (uint32_t)c.count; }       // the second mip (behind the first): list lengths

// maximum key over texels [i0, i1] x [j0, j1] of a face (a superset: the coarsest level at which the rectangle is at most
// 2 x 2 cells; four loads)
DXV_HD uint32_t dm_mip_max(const uint16_t* mip, uint32_t R, uint32_t face, uint32_t i0, uint32_t i1, uint32_t j0, uint32_t j1)
{
    uint32_t l = 0, off = 0, r = R;
    while (((i1 >> l) - (i0 >> l)) > 1u || ((j1 >> l) - (j0 >> l)) > 1u) { off += 6u * r * r; r >>= 1; ++l; }
    const uint16_t* base = mip + off + face * r * r;
    const uint32_t a0 = i0 >> l, a1 = i1 >> l, b0 = j0 >> l, b1 = j1 >> l;
    uint32_t m = base[b0 * r + a0], t = base[b0 * r + a1];
    if (t > m) m = t;
    t = base[b1 * r + a0]; if (t > m) m = t;
    t = base[b1 * r + a1]; if (t > m) m = t;
    return m;
}

// Can a voxel whose centre lies in the box [x0, x1] x [y0, y1] x [z0, z1] (the hull of a brick's voxel centres; x0 <= x1 ...)
// hold a live ray, i.e. pass origin_leaves_root and dm_ray_start().live?  False negatives are not allowed, false positives
// cost a wave that finds nothing to do.  Every step bounds the per-voxel arithmetic through its monotonicity in fp32
// (correctly rounded operations are monotone): coordinates of one sign, |u| = |p_b| / |p_a| grows with |p_b| and falls
// with |p_a|, the texel index grows with u, rho grows with every |coordinate|, near = rho * 0.999f with rho.
//  * root box: on an axis whose coordinates are all of one sign, axis_leaves_root is monotone -- all of them leave iff the
//    one nearest to zero does;
//  * a box that straddles a centre plane (grids whose half is no multiple of the brick) is kept;
//  * faces: in one octant a box meets the cone of face A iff its corner with the largest |a| and smallest |b|, |c| lies in
//    it, and likewise for the tie-breaking order of dm_ray_point -- the faces present among its voxels are exactly the
//    faces of three of its corners; per present face the texel rectangle of the box comes from the extreme quotients;
//  * every ray of the box starts at or beyond rhoMin: dead iff every texel it can look into is empty or ends before
//    rhoMin * 0.999f.
// (the faces a box of one octant can look into, each with the rectangle of texels its rays can fall on: visit(face, i0, i1, j0, j1)
// returns true to stop; the box must not straddle a centre plane)
template <class Visit>
DXV_HD bool dm_box_faces(float x0, float x1, float y0, float y1, float z0, float z1, uint32_t R, Visit&& visit)
{
    const bool nx = x1 < 0.0f, ny = y1 < 0.0f, nz = z1 < 0.0f;
    const float xa = nx ? -x1 : x0, xb = nx ? -x0 : x1, ya = ny ? -y1 : y0, yb = ny ? -y0 : y1, za = nz ? -z1 : z0, zb = nz ? -z0 : z1;
    // rectangle of texels for numerator range [na, nb] (sign neg) over denominator range [da, db]
    auto range = [&](float na, float nb, bool neg, float da, float db, uint32_t& t0, uint32_t& t1) {
        const float lo = na / db, hi = nb / da;
        t0 = dm_texel(neg ? -hi : lo, R); t1 = dm_texel(neg ? -lo : hi, R);
    };
    uint32_t i0, i1, j0, j1;
    if (xb >= ya && xb >= za) {                                         // face X: u = y / |x|, v = z / |x|
        range(ya, yb, ny, xa, xb, i0, i1); range(za, zb, nz, xa, xb, j0, j1);
        if (visit(nx ? 1u : 0u, i0, i1, j0, j1)) return true;
    }
    if (!(xa >= yb && xa >= za) && yb >= za) {                          // face Y: u = z / |y|, v = x / |y|
        range(za, zb, nz, ya, yb, i0, i1); range(xa, xb, nx, ya, yb, j0, j1);
        if (visit(ny ? 3u : 2u, i0, i1, j0, j1)) return true;
    }
    if (!(xa >= ya && xa >= zb) && !(ya >= zb)) {                       // face Z: u = x / |z|, v = y / |z|
        range(xa, xb, nx, za, zb, i0, i1); range(ya, yb, ny, za, zb, j0, j1);
        if (visit(nz ? 5u : 4u, i0, i1, j0, j1)) return true;
    }
    return false;
}
DXV_HD bool dm_box_straddles(float x0, float x1, float y0, float y1, float z0, float z1)
{
    return !(x0 > 0.0f || x1 < 0.0f) || !(y0 > 0.0f || y1 < 0.0f) || !(z0 > 0.0f || z1 < 0.0f);
}
DXV_HD bool dm_box_may_be_live(float x0, float x1, float y0, float y1, float z0, float z1, const float* rootLo, const float* rootHi,
                               const uint16_t* mip, uint32_t R)
{
    if ((x0 > 0.0f && axis_leaves_root(x0, rootLo[0], rootHi[0])) || (x1 < 0.0f && axis_leaves_root(x1, rootLo[0], rootHi[0]))) return false;
    if ((y0 > 0.0f && axis_leaves_root(y0, rootLo[1], rootHi[1])) || (y1 < 0.0f && axis_leaves_root(y1, rootLo[1], rootHi[1]))) return false;
    if ((z0 > 0.0f && axis_leaves_root(z0, rootLo[2], rootHi[2])) || (z1 < 0.0f && axis_leaves_root(z1, rootLo[2], rootHi[2]))) return false;
    if (dm_box_straddles(x0, x1, y0, y1, z0, z1)) return true;          // straddles a centre plane
    const bool nx = x1 < 0.0f, ny = y1 < 0.0f, nz = z1 < 0.0f;
    const float xa = nx ? -x1 : x0, ya = ny ? -y1 : y0, za = nz ? -z1 : z0;
    const float rhoMin = __builtin_sqrtf((xa * xa + ya * ya) + za * za), nearMin = rhoMin * 0.999f;
    return dm_box_faces(x0, x1, y0, y1, z0, z1, R, [&](uint32_t face, uint32_t i0, uint32_t i1, uint32_t j0, uint32_t j1) {
        const uint32_t key = dm_mip_max(mip, R, face, i0, i1, j0, j1);
        return key != 0u && !(half_bits_to_float(key) < nearMin);
    });
}
// The longest list any ray of the box can look into (an upper bound: the same rectangles through the max-mip of the texels' entry
// counts, which lies behind the first mip in memory).  Not a matter of results: it decides which bricks a launch starts with --
// a brick is as long as its longest list, one in a hundred takes three to seven times the mean, and a launch whose last bricks
// are of that kind ends with a handful of waves on an idle GPU (k_plan_bricks).  Boxes that straddle a centre plane: 0.
DXV_HD uint32_t dm_box_max_count(float x0, float x1, float y0, float y1, float z0, float z1, const uint16_t* countMip, uint32_t R)
{
    if (dm_box_straddles(x0, x1, y0, y1, z0, z1)) return 0u;
    uint32_t most = 0;
    (void)dm_box_faces(x0, x1, y0, y1, z0, z1, R, [&](uint32_t face, uint32_t i0, uint32_t i1, uint32_t j0, uint32_t j1) {
        const uint32_t c = dm_mip_max(countMip, R, face, i0, i1, j0, j1);
        if (c > most) most = c;
        return false;
    });
    return most;
}
// memory of the two mips, the per-level "long list" words behind them (16 words) and the build's scratch behind those (dirmap.hip:
// k_dm_mip_tiles leaves (sum, non-empty cells) per tile and level there for k_dm_mip_top), 16-bit words
DXV_HD uint32_t dm_mip_partials_at(uint32_t R) { return (2u * dm_mip_words(R) + 16u + 3u) & ~3u; }
DXV_HD uint32_t dm_mip_buffer_words(uint32_t R)
{
    const uint32_t tile = R < 32u ? R : 32u, tiles = 6u * (R / tile) * (R / tile);
    return dm_mip_partials_at(R) + 4u * tiles * 8u;                   // (two 32-bit words per tile and level, up to 8 levels inside a tile)
}
// the level of the count mip whose cells are about the patch of texels a 4^3-voxel brick of an N^3 grid looks into
// (4 voxels of 2 / N at a typical distance of 0.7 from the centre: ~5.6 R / N texels across)
constexpr uint32_t kDmHeavyLevelMin = 2u;           // (the levels below have no "long list" word: k_dm_heavy_thresholds)
DXV_HD uint32_t dm_heavy_level(uint32_t R, uint32_t N)
{
    uint32_t l = 0;
    while ((1u << (l + 1u)) * N <= 8u * R && l + 1u < dm_mip_levels(R)) ++l;      // 2^l <= 8 R / N < 2^(l + 1):  512 / 512 -> 3, 512 / 256 -> 4, 512 / 1024 -> 2
    const uint32_t top = dm_mip_levels(R) - 1u;
    return l < kDmHeavyLevelMin ? (kDmHeavyLevelMin < top ? kDmHeavyLevelMin : top) : l;
}

// the hull of the voxel centres of brick (bx, by, bz) of 4 x 4 x 4 voxels in a partition's local brick grid (x0 <= x1 ...; y falls
// with iy, hlsl:49).  Local slice lz <-> global slice: global_slice (dxv_math.h);
// the map is increasing, so the hull's z range comes from the brick's first and last slice.
DXV_HD void dm_brick_hull(uint32_t N, uint32_t nz, uint32_t z0, uint32_t zBlock, uint32_t zShift, uint32_t zPeriod, uint32_t bx, uint32_t by,
                          uint32_t bz, float& x0, float& x1, float& y0, float& y1, float& zlo, float& zhi)
{
    const uint32_t ix0 = bx * 4u, iy0 = by * 4u, lz0 = bz * 4u;
    const uint32_t ix1 = ix0 + 3u < N ? ix0 + 3u : N - 1u, iy1 = iy0 + 3u < N ? iy0 + 3u : N - 1u, lz1 = lz0 + 3u < nz ? lz0 + 3u : nz - 1u;
    const uint32_t iz0 = global_slice(z0, nz, zBlock, zShift, zPeriod, lz0), iz1 = global_slice(z0, nz, zBlock, zShift, zPeriod, lz1);
    ray_origin(N, ix0, iy1, iz0, x0, y0, zlo);
    ray_origin(N, ix1, iy0, iz1, x1, y1, zhi);
}

// next float towards +inf / -inf (finite inputs)
DXV_HD float dm_up(float x)
{
    if (x == 0.0f) return 1.401298464e-45f;
    const uint32_t b = __builtin_bit_cast(uint32_t, x);
    return __builtin_bit_cast(float, x > 0.0f ? b + 1u : b - 1u);
}
DXV_HD float dm_down(float x) { return -dm_up(-x); }

// The lateral bound of ONE whole projected triangle (the header's derivation, steps 1 - 6): how far outside an edge line, and how
// far outside the bounding box of its projected vertices, the direction point of a ray that leaf_reference accepts can lie, in
// face coordinates.  tri: the triangle in the face's coordinates (b, c, depth), all depths >= dmin >= 64 delta.  Returns 1e30
// where the derivation does not hold (coordinates beyond the unit cube, a projection that is (nearly) edge-on or degenerate, a
// smallest projected altitude below twice the bound): the caller keeps the 2^-15 pad there.
DXV_HD double dm_lateral_pad(const double (*tri)[3], double dmin)
{
    const double none = 1e30, u = 5.9604644775390625e-8;                 // (u = 2^-24: a rounded fp32 result is within u of its size)
    double lo[3], hi[3], big = 0.0;
    for (int k = 0; k < 3; ++k) { lo[k] = hi[k] = tri[0][k]; }
    for (int i = 0; i < 3; ++i)
        for (int k = 0; k < 3; ++k) {
            const double x = tri[i][k];
            if (x < lo[k]) lo[k] = x;
            if (x > hi[k]) hi[k] = x;
            if (__builtin_fabs(x) > big) big = __builtin_fabs(x);
        }
    if (!(big <= 1.0)) return none;                                     // step 1 takes |v - o| <= 2 per axis
    const double diag = __builtin_sqrt((hi[0] - lo[0]) * (hi[0] - lo[0]) + (hi[1] - lo[1]) * (hi[1] - lo[1]) + (hi[2] - lo[2]) * (hi[2] - lo[2]));
    // step 2: sheared vertices within Dm of the ray (slab test of the box padded by 2^-16, taken as 2^-15 for the slab's own roundings)
    const double Dm = 1.7321 * (diag + 3.4642 * (double)kDmDelta);
    // step 1: one sheared coordinate -- two differences of at most 2 each, one fused step of at most 4: the sizes the unit cube allows
    const double E = 8.0 * u;
    // steps 3, 4: what a computed edge function can differ by from the exact one of the true radial line
    const double e1 = 2.8285 * E * Dm + 2.0 * E * E + 2.01 * u * Dm * Dm + 15.0 * u * diag;
    // step 5: face coordinates
    double pu[3], pv[3];
    for (int i = 0; i < 3; ++i) { pu[i] = tri[i][0] / tri[i][2]; pv[i] = tri[i][1] / tri[i][2]; }
    const double ax = pu[1] - pu[0], ay = pv[1] - pv[0], bx = pu[2] - pu[0], by = pv[2] - pv[0], cx = pu[2] - pu[1], cy = pv[2] - pv[1];
    const double area2 = __builtin_fabs(ax * by - ay * bx);
    const double la = ax * ax + ay * ay, lb = bx * bx + by * by, lc = cx * cx + cy * cy;
    if (!(area2 > 1e-3 * (la + lb)) || !(la + lb > 1e-24)) return none;  // (nearly) edge-on: the threshold of dm_texel_test and dm_local_radial
    double l2 = la > lb ? la : lb;
    if (lc > l2) l2 = lc;
    const double hmin = area2 / __builtin_sqrt(l2);                      // smallest altitude of the projected triangle
    // step 6: the corner of the pushed-out edges, 1 % for this function's own double arithmetic
    const double own = 1.01 * 2.0 * e1 / (dmin * dmin * hmin);
    if (!(own < 0.5 * hmin)) return none;                               // below this altitude all three signs could flip together
    return own;
}

// Footprint of triangle tp on one face, or false when it cannot be seen through that face.
// Builder side only (one call per triangle and face): double precision, nothing canonical here --
// the result only has to be a superset.
struct DirFootprint { float u0, u1, v0, v1, r0, r1, pad, px[3], py[3], pw[3]; bool hasTri; float padWide; bool lateral; };   // (padWide: the 2^-15 pad; lateral: made with option lateralpad on)

// The polygon a face sees of a triangle (its vertices in the face's own coordinates b, c, +-a) -> footprint.  FIXED = 3: the
// triangle itself, whole inside the face's frustum -- by far the common case; all loops have constant bounds then and the
// polygon stays in registers (the general case indexes it dynamically: scratch memory on the device).
template <int FIXED>
DXV_HD void dm_footprint_finish(const double (*poly)[3], int n, const double (*tri)[3], DirFootprint& out, bool lateral = true)
{
    const int m = FIXED ? FIXED : n;
    const double delta = (double)kDmDelta;
    double dmin = poly[0][2], rmax2 = 0.0;                        // (radii squared until the end: the root is monotone)
    for (int i = 0; i < m; ++i) {
        const double* q = poly[i];
        if (q[2] < dmin) dmin = q[2];
        const double r2 = q[0] * q[0] + q[1] * q[1] + q[2] * q[2];
        if (r2 > rmax2) rmax2 = r2;
    }
    const double full = kDmFrustum + 1.0 / 256.0;
    double u0 = -full, u1 = full, v0 = -full, v1 = full;
    out.hasTri = false; out.pad = 0.0f; out.padWide = 0.0f; out.lateral = lateral;
    for (int i = 0; i < 3; ++i) out.px[i] = out.py[i] = out.pw[i] = 0.0f;
    if (dmin >= 64.0 * delta) {
        u0 = v0 = 1e300; u1 = v1 = -1e300;
        for (int i = 0; i < m; ++i) {
            const double* q = poly[i];
            const double u = q[0] / q[2], v = q[1] / q[2];
            if (u < u0) u0 = u;
            if (u > u1) u1 = u;
            if (v < v0) v0 = v;
            if (v > v1) v1 = v;
        }
        // a point moved by delta sideways and in depth at depth >= dmin >= 64 delta, |u| <= 1.006:
        // du <= (1 + |u|) delta / (dmin - delta) <= 2.04 delta / dmin
        const double wide = 2.25 * delta / dmin + 1e-6;
        // ... and a whole, well-shaped projected triangle is held by its own bound instead (dm_lateral_pad; never the larger).  The box
        // stays the wide pad's: the record carries both pads and hands out the narrow box (dm_record_box)
        double pad = wide;
        if (FIXED == 3 && lateral) { const double own = dm_lateral_pad(tri, dmin) + 1e-6; if (own < pad) pad = own; }
        u0 -= wide; u1 += wide; v0 -= wide; v1 += wide;
        const bool cut = u0 < -full || v0 < -full || u1 > full || v1 > full;    // (a box cut to the face has no pad to take back)
        // the projected triangle itself, when all of it lies in front of the face plane: its edges, pushed out by the same
        // pad, bound the footprint too (the part cut off by the frustum's side planes only makes the polygon smaller)
        const double d0 = tri[0][2], d1 = tri[1][2], d2 = tri[2][2];           // (tri: the unclipped triangle in the face's coordinates)
        if (d0 >= 64.0 * delta && d1 >= 64.0 * delta && d2 >= 64.0 * delta) {
            const double dd[3] = {d0, d1, d2};
            for (int i = 0; i < 3; ++i) { out.px[i] = (float)(tri[i][0] / dd[i]); out.py[i] = (float)(tri[i][1] / dd[i]); out.pw[i] = (float)(1.0 / dd[i]); }
            out.hasTri = true;
            out.padWide = (float)(wide + 1e-6);                 // (+ the rounding of the stored vertices)
            out.pad = cut ? out.padWide : (float)(pad + 1e-6);
            if (!(out.pad < out.padWide)) { out.pad = out.padWide; out.lateral = false; }
        }
        else out.lateral = false;
        if (u0 < -full) u0 = -full;
        if (v0 < -full) v0 = -full;
        if (u1 > full) u1 = full;
        if (v1 > full) v1 = full;
    }
    // radial range: the farthest point of a convex polygon is a vertex; the nearest is the foot of the perpendicular from
    // the centre onto its plane when that lies inside the polygon, else the nearest point of its boundary.  (A tight near
    // radius matters twice: it is what culls entries behind a hit, and the thickest entry of a texel decides how far
    // behind a hit the scan of that texel goes on.)
    double rmin2 = 1e300;
    for (int i = 0; i < m; ++i) {                                      // nearest point of every edge (covers degenerate polygons)
        const double* A = poly[i];
        const double* B = poly[(i + 1) % m];
        const double d[3] = {B[0] - A[0], B[1] - A[1], B[2] - A[2]};
        const double dd = d[0] * d[0] + d[1] * d[1] + d[2] * d[2];
        double w = dd > 0.0 ? -(A[0] * d[0] + A[1] * d[1] + A[2] * d[2]) / dd : 0.0;
        w = w < 0.0 ? 0.0 : w > 1.0 ? 1.0 : w;
        const double x = A[0] + w * d[0], y = A[1] + w * d[1], z = A[2] + w * d[2];
        const double dist2 = x * x + y * y + z * z;
        if (dist2 < rmin2) rmin2 = dist2;
    }
    if (m >= 3) {
        // plane through the polygon (its vertices are coplanar: clipped from one triangle), in the polygon's own coordinates
        const double* A = poly[0];
        double nx = 0.0, ny = 0.0, nz = 0.0;
        for (int i = 1; i + 1 < m; ++i) {                              // summed fan normals: robust for thin clips
            const double* B = poly[i];
            const double* C = poly[i + 1];
            const double e1[3] = {B[0] - A[0], B[1] - A[1], B[2] - A[2]}, e2[3] = {C[0] - A[0], C[1] - A[1], C[2] - A[2]};
            nx += e1[1] * e2[2] - e1[2] * e2[1]; ny += e1[2] * e2[0] - e1[0] * e2[2]; nz += e1[0] * e2[1] - e1[1] * e2[0];
        }
        const double nn = nx * nx + ny * ny + nz * nz;
        if (nn > 1e-60) {
            const double k = (nx * A[0] + ny * A[1] + nz * A[2]) / nn;
            const double P[3] = {k * nx, k * ny, k * nz};               // foot of the perpendicular from the centre
            bool inside = true;
            for (int i = 0; i < m && inside; ++i) {
                const double* E = poly[i];
                const double* F = poly[(i + 1) % m];
                const double d[3] = {F[0] - E[0], F[1] - E[1], F[2] - E[2]}, q[3] = {P[0] - E[0], P[1] - E[1], P[2] - E[2]};
                const double cx = d[1] * q[2] - d[2] * q[1], cy = d[2] * q[0] - d[0] * q[2], cz = d[0] * q[1] - d[1] * q[0];
                // same turn as the polygon's own orientation (the fan normal).  The clip leaves coincident vertices behind
                // (an edge through a frustum corner is cut twice at one point): such an edge's product is rounding noise of
                // either sign, so the test forgives 1e-10 of the operands' scale.  Erring towards "inside" is the safe side:
                // the distance to the plane never exceeds the distance to any point of the polygon.
                const double qq = q[0] * q[0] + q[1] * q[1] + q[2] * q[2];
                inside = cx * nx + cy * ny + cz * nz >= -1e-10 * (1.0 + rmax2) * __builtin_sqrt(qq * nn);
            }
            const double dist2 = k * k * nn;
            if (inside && dist2 < rmin2) rmin2 = dist2;
        }
    }
    double rmin = __builtin_sqrt(rmin2), rmax = __builtin_sqrt(rmax2);
    rmin *= 1.0 - 1e-6;
    rmin -= 4.0 * delta;
    if (rmin < 0.0) rmin = 0.0;
    rmax += 4.0 * delta;
    out.u0 = (float)u0; out.u1 = (float)u1; out.v0 = (float)v0; out.v1 = (float)v1;
    out.r0 = (float)rmin; out.r1 = (float)rmax;
    // float conversion rounds to nearest: one more ulp outward
    out.u0 = dm_down(out.u0); out.v0 = dm_down(out.v0); out.u1 = dm_up(out.u1); out.v1 = dm_up(out.v1);
    out.r0 = out.r0 > 0.0f ? dm_down(out.r0) : 0.0f;
    out.r1 = dm_up(out.r1);
}


DXV_HD bool dm_footprint(const TriPos& tp, uint32_t face, DirFootprint& out, bool lateral = true)
{
    const uint32_t a = face >> 1, b = (a + 1u) % 3u, c = (a + 2u) % 3u;
    const double s = (face & 1u) ? -1.0 : 1.0;
    // the triangle in the face's coordinates (b, c, +-a); the axes are picked by selects, not by indexing (no scratch memory)
    const float X[3] = {tp.v0.x, tp.v1.x, tp.v2.x}, Y[3] = {tp.v0.y, tp.v1.y, tp.v2.y}, Z[3] = {tp.v0.z, tp.v1.z, tp.v2.z};
    double tri[3][3];
    for (int i = 0; i < 3; ++i) {
        tri[i][0] = b == 0u ? X[i] : b == 1u ? Y[i] : Z[i];
        tri[i][1] = c == 0u ? X[i] : c == 1u ? Y[i] : Z[i];
        tri[i][2] = s * (double)(a == 0u ? X[i] : a == 1u ? Y[i] : Z[i]);
    }
    const double delta = (double)kDmDelta;
    // the four side planes of the widened frustum, pushed out by the dilation: kF * d +- b + 2 delta >= 0
    const double planes[4][2] = {{1.0, 0.0}, {-1.0, 0.0}, {0.0, 1.0}, {0.0, -1.0}};
    // most (triangle, face) pairs end here: all three vertices outside one side plane (what the clip
    // below would find, without its arrays)
    bool allIn = true;
    for (int pl = 0; pl < 4; ++pl) {
        bool anyIn = false;
        for (int i = 0; i < 3; ++i) {
            const bool in = kDmFrustum * tri[i][2] + planes[pl][0] * tri[i][0] + planes[pl][1] * tri[i][1] + 2.0 * delta >= 0.0;
            anyIn = anyIn || in;
            allIn = allIn && in;
        }
        if (!anyIn) return false;
    }
    if (allIn) {                                                        // nothing to clip: the polygon is the triangle
        dm_footprint_finish<3>(tri, 3, tri, out, lateral);
        return true;
    }
    double poly[2][10][3];
    int n = 3, cur = 0;
    for (int i = 0; i < 3; ++i) for (int k = 0; k < 3; ++k) poly[0][i][k] = tri[i][k];
    for (int pl = 0; pl < 4 && n > 0; ++pl) {
        const double nb = planes[pl][0], nc = planes[pl][1];
        int m = 0;
        for (int i = 0; i < n; ++i) {
            const double* A = poly[cur][i];
            const double* B = poly[cur][(i + 1) % n];
            const double fa = kDmFrustum * A[2] + nb * A[0] + nc * A[1] + 2.0 * delta;
            const double fb = kDmFrustum * B[2] + nb * B[0] + nc * B[1] + 2.0 * delta;
            if (fa >= 0.0) { for (int k = 0; k < 3; ++k) poly[cur ^ 1][m][k] = A[k]; ++m; }
            if ((fa >= 0.0) != (fb >= 0.0)) {
                const double w = fa / (fa - fb);
                for (int k = 0; k < 3; ++k) poly[cur ^ 1][m][k] = A[k] + (B[k] - A[k]) * w;
                ++m;
            }
        }
        cur ^= 1;
        n = m;
    }
    if (n == 0) return false;
    dm_footprint_finish<0>(poly[cur], n, tri, out, lateral);
    return true;
}

// the record of a (triangle, face) pair; u0 > u1 when there is no footprint
DXV_HD DirRecord dm_record(const DirFootprint& f)
{
    DirRecord r;
    r.u0 = f.u0; r.u1 = f.u1; r.v0 = f.v0; r.v1 = f.v1;
    r.rr = (uint32_t)half_down(f.r0) | ((uint32_t)half_up(f.r1) << 16);
    r.hasTri = f.hasTri ? 1u : 0u; r.pad = f.pad;
    // (made with the per-record bound: the 2^-15 pad rides along -- a pad is a float in [2^-63, 2): its top three bits are 001)
    const uint32_t wideBits = __builtin_bit_cast(uint32_t, f.padWide);
    if (f.hasTri && f.lateral && (wideBits >> 29) == 1u) r.hasTri |= kDmRecLateral | (wideBits << 3);
    for (int i = 0; i < 3; ++i) { r.px[i] = f.px[i]; r.py[i] = f.py[i]; r.pw[i] = f.pw[i]; }
    return r;
}
DXV_HD DirRecord dm_record(const TriPos& tp, uint32_t face, bool lateral = true)
{
    DirFootprint f;
    if (!dm_footprint(tp, face, f, lateral)) {
        DirRecord r;
        r.u0 = 1.0f; r.u1 = 0.0f; r.v0 = 1.0f; r.v1 = 0.0f; r.rr = 0u; r.hasTri = 0u; r.pad = 0.0f;
        for (int i = 0; i < 3; ++i) r.px[i] = r.py[i] = r.pw[i] = 0.0f;
        return r;
    }
    return dm_record(f);
}

// texel rectangle [i0, i1] x [j0, j1] of a record (false: none)
DXV_HD bool dm_rect(const DirRecord& e, uint32_t R, uint32_t& i0, uint32_t& i1, uint32_t& j0, uint32_t& j1)
{
    if (e.u0 > e.u1) return false;
    const DirBox b = dm_record_box(e);
    if (b.u1 < -1.0f || b.u0 > 1.0f || b.v1 < -1.0f || b.v0 > 1.0f) return false;      // rays only have |u|, |v| <= 1
    i0 = dm_texel(b.u0, R); i1 = dm_texel(b.u1, R); j0 = dm_texel(b.v0, R); j1 = dm_texel(b.v1, R);
    return true;
}

// Radial range of a record INSIDE texel (i, j), as halfs rounded outward: a triangle that spans several texels (every triangle of
// a coarse mesh, of a soup) is radially much thinner over one of them than as a whole, and the radial range is what culls an entry
// before its triangle is fetched, what orders a texel's list and what lets a scan stop behind a hit.
// 1 / depth along the face axis is LINEAR in the face coordinates (u, v) over the triangle's plane: w(u, v) = pw0 + gu (u - px0)
// + gv (v - py0), its extremes over a rectangle lie at the corners, and a point of the plane in direction (u, v) has radius
// sqrt(1 + u^2 + v^2) / w(u, v).  The rectangle is the texel cut by the record's box, widened by the record's pad (the rays of the
// texel, the dilated triangle's outline); the plane extrapolated beyond the triangle only widens the range.  Points within the
// dilation delta of the plane lie within delta rho / |d| of it along a ray (d: the plane's distance from the centre, 1 / d^2 =
// w(0, 0)^2 + gu^2 + gv^2): taken twice, plus the whole footprint's own margins.  The result is cut with the whole footprint's
// range; records without a projected triangle, seen edge-on, or whose plane passes the centre keep that range.
// Which texels of a record's rectangle get an entry at all.  The rectangle is the bounding box of the footprint: a triangle fills
// half of its box, and a quarter to a third of the (triangle, texel) pairs of a mesh are texels that lie entirely outside one
// edge of the projected, dilated triangle -- entries no ray could ever select (measured on the host: 28 % bunny, 35 % dragon, 38 % a
// soup, 11 % a mesh of texel-sized triangles).  dm_texel_test makes the three edge functions of a record once (inside edge k <=>
// nx u + ny v + c >= 0, the dilation `pad` and every rounding of this single-precision arithmetic on the safe side of c);
// dm_texel_outside says whether a texel's rectangle (widened by more than the rays' own rounding) lies wholly outside one of them.
// Counting pass, key pass and the host's replica call the same two functions.  Records without a projected triangle, seen
// (nearly) edge-on, or with more than kDmTexelTestMax texels keep their whole rectangle.
constexpr uint32_t kDmTexelTestMax = 1024u;          // (beyond: a triangle close to the centre -- rare, and one thread walks the rectangle in the counting pass)
struct DirTexelTest { float nx[3], ny[3], c[3]; bool on; };
DXV_HD DirTexelTest dm_texel_test(const DirRecord& rec, uint32_t texels)
{
    DirTexelTest t;
    t.on = false;
    for (int k = 0; k < 3; ++k) { t.nx[k] = 0.0f; t.ny[k] = 0.0f; t.c[k] = 0.0f; }
    // (a strip of two or three texels is touched in all of them -- by the 2^-15 pad.  A record with a bound of its own is tested whatever
    // its rectangle: the smaller pad's rectangle is the smaller one, and a test that came on with the area would let the wide pad
    // drop a texel the narrow pad keeps)
    if (!(rec.hasTri & 1u) || texels < ((rec.hasTri & kDmRecLateral) ? 1u : 4u) || texels > kDmTexelTestMax) return t;
    const float ax = rec.px[1] - rec.px[0], ay = rec.py[1] - rec.py[0], bx = rec.px[2] - rec.px[0], by = rec.py[2] - rec.py[0];
    const float area2 = ax * by - ay * bx;
    const float scale = (ax * ax + ay * ay) + (bx * bx + by * by);
    if (!(__builtin_fabsf(area2) > 1e-3f * scale) || !(scale > 1e-24f)) return t;
    const float sgn = area2 > 0.0f ? 1.0f : -1.0f;
    for (int k = 0; k < 3; ++k) {
        const int k1 = k == 2 ? 0 : k + 1;
        const float ex = rec.px[k1] - rec.px[k], ey = rec.py[k1] - rec.py[k];
        const float nx = -ey * sgn, ny = ex * sgn;                      // inward normal (not unit: |n| <= |nx| + |ny| pays for that)
        const float l1 = __builtin_fabsf(nx) + __builtin_fabsf(ny);
        const float px = rec.px[k] * nx, py = rec.py[k] * ny;
        t.nx[k] = nx; t.ny[k] = ny;
        t.c[k] = -(px + py) + (rec.pad + 1e-5f) * l1 + 1e-6f * (__builtin_fabsf(px) + __builtin_fabsf(py)) + 1e-30f;
    }
    t.on = true;
    return t;
}
DXV_HD bool dm_texel_outside(const DirTexelTest& t, uint32_t R, uint32_t i, uint32_t j)
{
    if (!t.on) return false;
    const float inv = 2.0f / (float)R;                                  // (R a power of two: exact)
    const float u0 = (float)i * inv - 1.0f - 4e-6f, u1 = (float)(i + 1u) * inv - 1.0f + 4e-6f;
    const float v0 = (float)j * inv - 1.0f - 4e-6f, v1 = (float)(j + 1u) * inv - 1.0f + 4e-6f;
    for (int k = 0; k < 3; ++k) {
        const float pu = t.nx[k] > 0.0f ? u1 : u0, pv = t.ny[k] > 0.0f ? v1 : v0;       // the corner farthest inside edge k
        const float a = t.nx[k] * pu, b = t.ny[k] * pv;
        if ((a + b) + t.c[k] + 1e-6f * (__builtin_fabsf(a) + __builtin_fabsf(b)) < 0.0f) return true;
    }
    return false;
}

constexpr uint32_t kDmLocalRadialFrom = 12u;         // footprints of more texels than this get per-texel radial ranges
// hasTri bit 1: the record's footprint covers more than kDmLocalRadialFrom texels of the map the lists are built on (`texels`: the
// area of its rectangle there) and has a projected triangle -- set by whoever makes the record for a map (k_dm_records, hostcheck)
DXV_HD void dm_record_on_map(DirRecord& rec, uint32_t texels)
{
    if ((rec.hasTri & 1u) && texels > kDmLocalRadialFrom && texels <= kDmTexelTestMax) rec.hasTri |= 2u;
}
DXV_HD void dm_local_radial(const DirRecord& rec, uint32_t R, uint32_t i, uint32_t j, uint32_t& r0h, uint32_t& r1h)
{
    r0h = rec.rr & 0xffffu; r1h = rec.rr >> 16;
    // (a footprint of a few texels is hardly thinner over one of them: the whole range, for nothing -- every record of a mesh whose
    // triangles are as small as the texels ends here; the flag is set where the record's rectangle on this map is known: dm_record_on_map)
    if (!(rec.hasTri & 2u)) return;
    // (single precision throughout -- this runs once per entry in two passes of the build -- with every rounding paid for below: the fit
    // of a triangle seen within 1e-3 of edge-on is not trusted at all, the fitted w carries 2e-3 of its own variation over the
    // rectangle and 1e-5 of its size, the radii 3e-5 of theirs.  Plain IEEE operations, no contraction: host and device agree.)
    const float ax = rec.px[1] - rec.px[0], ay = rec.py[1] - rec.py[0], aw = rec.pw[1] - rec.pw[0];
    const float bx = rec.px[2] - rec.px[0], by = rec.py[2] - rec.py[0], bw = rec.pw[2] - rec.pw[0];
    const float det = ax * by - ay * bx;
    const float scale = (ax * ax + ay * ay) + (bx * bx + by * by);
    if (!(__builtin_fabsf(det) > 1e-3f * scale) || !(scale > 1e-24f)) return;   // seen (nearly) edge-on, or degenerate: no plane to speak of
    const float gu = (aw * by - bw * ay) / det, gv = (bw * ax - aw * bx) / det;
    const float w00 = rec.pw[0] - gu * rec.px[0] - gv * rec.py[0];
    const float invd = __builtin_sqrtf(w00 * w00 + gu * gu + gv * gv);
    if (!(invd * kDmDelta < 0.125f)) return;                                    // the plane passes (nearly) through the centre
    const float eps = rec.pad + 4e-6f;
    float ua = 2.0f * (float)i / (float)R - 1.0f, ub = 2.0f * (float)(i + 1u) / (float)R - 1.0f;
    float va = 2.0f * (float)j / (float)R - 1.0f, vb = 2.0f * (float)(j + 1u) / (float)R - 1.0f;
    const DirBox box = dm_record_box(rec);
    if (box.u0 > ua) ua = box.u0;
    if (box.u1 < ub) ub = box.u1;
    if (box.v0 > va) va = box.v0;
    if (box.v1 < vb) vb = box.v1;
    ua -= eps; ub += eps; va -= eps; vb += eps;
    if (!(ua <= ub && va <= vb)) return;
    const float w0 = w00 + gu * ua + gv * va, w1 = w00 + gu * ub + gv * va, w2 = w00 + gu * ua + gv * vb, w3 = w00 + gu * ub + gv * vb;
    float wmin = w0 < w1 ? w0 : w1, wmax = w0 > w1 ? w0 : w1;
    if (w2 < wmin) wmin = w2;
    if (w3 < wmin) wmin = w3;
    if (w2 > wmax) wmax = w2;
    if (w3 > wmax) wmax = w3;
    const float terms = __builtin_fabsf(w00) + __builtin_fabsf(gu) * (__builtin_fabsf(ua) > __builtin_fabsf(ub) ? __builtin_fabsf(ua) : __builtin_fabsf(ub)) +
                        __builtin_fabsf(gv) * (__builtin_fabsf(va) > __builtin_fabsf(vb) ? __builtin_fabsf(va) : __builtin_fabsf(vb));
    const float slack = 2e-3f * (wmax - wmin) + 1e-5f * terms;
    wmin -= slack; wmax += slack;
    const float ulo = ua > 0.0f ? ua : ub < 0.0f ? -ub : 0.0f, vlo = va > 0.0f ? va : vb < 0.0f ? -vb : 0.0f;
    const float uhi = -ua > ub ? -ua : ub, vhi = -va > vb ? -va : vb;
    const float thick = 2.0f * kDmDelta * invd + 3e-5f;
    if (wmax > 0.0f) {
        float rmin = __builtin_sqrtf(1.0f + ulo * ulo + vlo * vlo) / wmax;
        rmin = rmin * (1.0f - thick) - 4.0f * kDmDelta;
        if (rmin > 0.0f) { const uint32_t h = half_down(rmin); if (h > r0h) r0h = h; }
    }
    if (wmin > 1e-6f) {
        float rmax = __builtin_sqrtf(1.0f + uhi * uhi + vhi * vhi) / wmin;
        rmax = rmax * (1.0f + thick) + 4.0f * kDmDelta;
        if (rmax < 60000.0f) { const uint32_t h = half_up(rmax); if (h < r1h) r1h = h; }
    }
    if (r0h > r1h) r0h = r1h;                                                   // (cannot happen for a range that holds a point; keeps the words ordered)
}

// The entry of a record in texel (i, j) of its rectangle: the box cut to the texel in local cells, the radial word, and
// the edge of the projected triangle that removes most of that box.
// Edge arithmetic (builder side, double): inside the dilated triangle means (p - P_k) . n_k + pad >= 0 for the unit inward
// normal n_k of every edge k.  With texel-local coordinates X, Y (u = 2 i / R - 1 + X / (64 R)) that is A X + B Y + C >= 0;
// scaled so that the larger of |A|, |B| is 127 (ka, kb) and rounded to bytes a, b.  The bytes multiply cells counted from the
// texel's CENTRE: a ray in integer cell (x, y) is anywhere in [x, x + 1) x [y, y + 1), X = 64 + x' + fx with x' = x - 64 in
// [-64, 63] and fx in [0, 1), so the scaled function is  ka x' + kb y' + (C + 64 (ka + kb)) + ka fx + kb fy:  the constant is the
// edge function AT THE CENTRE, ka fx + kb fy is at most |ka| + |kb| (position inside the cell), and a x' + b y' falls short of
// ka x' + kb y' by at most 0.5 (|x'| + |y'|) <= 64 (rounding of a and b) -- half of what cells counted from the corner, up to
// 127 each way, cost.  c takes all of that + 13 for the ray's own float arithmetic, so the byte test passes wherever the real
// one does (it gives away one and a half to three cells of 128).  Centred, |a x' + b y'| <= 2 * 127 * 64 = 16,256: every line
// that crosses the texel has a c the two bytes (127 c1 + c2) hold -- from the corner a diagonal edge beyond the centre, a quad's
// hypotenuse, had none and was clamped or dropped.  What is still out of range cuts nothing (c >= 16,256: dropped) or all of
// the texel (c < -16,256: clamped, never stricter).
DXV_HD DirEntry dm_local_entry(const DirRecord& rec, uint32_t R, uint32_t i, uint32_t j, uint32_t tri)
{
    DirEntry e;
    e.tri = tri;
    uint32_t r0h, r1h;
    dm_local_radial(rec, R, i, j, r0h, r1h);
    e.rr = ((0x7fffu - r0h) | (r1h << 16)) | 0x80008000u;
    uint32_t t0, c0, t1, c1, x0, x1, y0, y1;
    const DirBox box = dm_record_box(rec);
    dm_local(box.u0, R, t0, c0); dm_local(box.u1, R, t1, c1);
    x0 = t0 < i ? 0u : c0; x1 = t1 > i ? kDmCells - 1u : c1;
    dm_local(box.v0, R, t0, c0); dm_local(box.v1, R, t1, c1);
    y0 = t0 < j ? 0u : c0; y1 = t1 > j ? kDmCells - 1u : c1;
    // (the 2^-15 pad and its box cut to the texel: what the choice of the edge below goes by -- the record's own where it has no other)
    const double wide = (double)dm_wide_pad(rec);
    uint32_t wx0 = x0, wx1 = x1, wy0 = y0, wy1 = y1;
    if (rec.hasTri & kDmRecLateral) {
        dm_local(rec.u0, R, t0, c0); dm_local(rec.u1, R, t1, c1);
        wx0 = t0 < i ? 0u : c0; wx1 = t1 > i ? kDmCells - 1u : c1;
        dm_local(rec.v0, R, t0, c0); dm_local(rec.v1, R, t1, c1);
        wy0 = t0 < j ? 0u : c0; wy1 = t1 > j ? kDmCells - 1u : c1;
    }
    e.box = x0 | (y0 << 8) | ((kDmCells - 1u - x1) << 16) | ((kDmCells - 1u - y1) << 24);
    e.edge = 0u;
    if (!(rec.hasTri & 1u)) return e;
    const double area2 = ((double)rec.px[1] - rec.px[0]) * ((double)rec.py[2] - rec.py[0]) - ((double)rec.py[1] - rec.py[0]) * ((double)rec.px[2] - rec.px[0]);
    if (!(__builtin_fabs(area2) > 1e-14)) return e;                     // seen edge-on: the box has to do
    const double sgn = area2 > 0.0 ? 1.0 : -1.0;
    const double ou = 2.0 * i / R - 1.0, ov = 2.0 * j / R - 1.0, perCell = 1.0 / (64.0 * R);
    int bestCut = 0;
    for (int k = 0; k < 3; ++k) {
        const double ex = (double)rec.px[(k + 1) % 3] - rec.px[k], ey = (double)rec.py[(k + 1) % 3] - rec.py[k];
        const double len2 = ex * ex + ey * ey;
        if (!(len2 > 1e-24)) continue;
        // inward normal, unit to 3e-7 (single-precision root and reciprocal: the test is homogeneous in the normal except for
        // `pad`, which carries 10 % of slack)
        const double rl = (double)(1.0f / __builtin_sqrtf((float)len2)) * sgn;
        const double nx = -ey * rl, ny = ex * rl;
        const double A = nx * perCell, B = ny * perCell;
        const double C0 = (ou - rec.px[k]) * nx + (ov - rec.py[k]) * ny, C = C0 + rec.pad, Cwide = C0 + wide;
        const double big = __builtin_fabs(A) > __builtin_fabs(B) ? __builtin_fabs(A) : __builtin_fabs(B);
        const double sc = (double)(127.0f / (float)big);                // (one scale for A, B and C: its last bits do not matter)
        const double ka = A * sc, kb = B * sc;
        const int a = (int)__builtin_floor(ka + 0.5), b = (int)__builtin_floor(kb + 0.5);
        double cd = __builtin_ceil(C * sc + 64.0 * (ka + kb) + __builtin_fabs(ka) + __builtin_fabs(kb) + 64.0 + 13.0);
        const double cdWide = __builtin_ceil(Cwide * sc + 64.0 * (ka + kb) + __builtin_fabs(ka) + __builtin_fabs(kb) + 64.0 + 13.0);
        if (!(cdWide < 16256.0)) continue;                               // this edge cuts nothing off the texel
        if (cd < -16256.0) cd = -16256.0;                               // (never stricter: safe)
        const int c = (int)cd, cw = (int)(cdWide < -16256.0 ? -16256.0 : cdWide);
        const int c1b = c / 127, c2b = c - 127 * c1b;                   // truncation: |c2b| < 127
        // how much of the box does it remove?  Nothing when the box's corner farthest outside is still inside; else 3 x 3 samples
        // (cells from the centre, as the ray brings them).  Asked of the constant of the 2^-15 pad and of that pad's box: the edge stored
        // is the same whichever pad the record was made with (dm_wide_pad)
        const int half = (int)kDmCells / 2;
        const int worst = a * ((int)(a < 0 ? wx1 : wx0) - half) + b * ((int)(b < 0 ? wy1 : wy0) - half) + cw;
        if (worst >= 0) continue;
        int cut = 1;
        for (int sy = 0; sy < 3; ++sy)
            for (int sx = 0; sx < 3; ++sx) {
                const int x = (int)wx0 + (int)((wx1 - wx0) * (2 * sx + 1) / 6) - half, y = (int)wy0 + (int)((wy1 - wy0) * (2 * sy + 1) / 6) - half;
                if (a * x + b * y + cw < 0) ++cut;
            }
        if (cut > bestCut) {
            bestCut = cut;
            e.edge = (uint32_t)(uint8_t)(int8_t)a | ((uint32_t)(uint8_t)(int8_t)b << 8) | ((uint32_t)(uint8_t)(int8_t)c1b << 16) | ((uint32_t)(uint8_t)(int8_t)c2b << 24);
        }
    }
    return e;
}

// List order: by texel, inside a texel by far radius r1 ascending (then by triangle).  Sort key:
//   cell (cellBits = bits of 6 R R - 1) | r1 as half (16 bits; positive halfs order like integers) | triangle (the rest)
struct DirKeyLayout { uint32_t cellBits, triBits; };
DXV_HD DirKeyLayout dm_key_layout(uint32_t R)
{
    DirKeyLayout k;
    k.cellBits = 1u;
    while ((6ull * R * R - 1ull) >> k.cellBits) ++k.cellBits;
    k.triBits = 64u - 16u - k.cellBits;
    return k;
}
DXV_HD uint64_t dm_key(const DirKeyLayout& k, uint32_t cell, uint16_t r1, uint32_t tri)
{
    return ((uint64_t)cell << (64u - k.cellBits)) | ((uint64_t)r1 << k.triBits) | (uint64_t)tri;
}
DXV_HD uint32_t dm_key_cell(const DirKeyLayout& k, uint64_t key) { return (uint32_t)(key >> (64u - k.cellBits)); }
DXV_HD uint32_t dm_key_tri(const DirKeyLayout& k, uint64_t key) { return (uint32_t)(key & ((1ull << k.triBits) - 1ull)); }

constexpr uint32_t kDmCoopLanes = 2u, kDmCoopMin = 24u;     // the cooperative scan of a lone lane's long list (trace_reference_dm_from)
// Diagnostic build (-DDXV_PHASE_TIMES, tools/phase_times.py): where a brick's TIME goes -- 100 MHz ticks between stamps of the wave's own
// instruction stream, summed over all bricks per phase: [0] ray set-up and the texel's cell, [1] start search, [2] scan rounds,
// [3] direction / shear at a flush, [4] triangle rounds, [5] predicate and stores; [6] bricks, [7] scan rounds counted, [8] triangle
// rounds counted, [9] flushes.  A stall on a load is charged to the phase that first uses the value.
#if defined(DXV_PHASE_TIMES) && defined(__HIPCC__)
constexpr uint32_t kPhaseSlots = 1u << 16;                   // (a workgroup adds to the slot of its number: no two waves in flight share a word for long)
static __device__ unsigned long long g_dxvPhase[kPhaseSlots * 16u];
#endif
#if defined(DXV_PHASE_TIMES) && defined(__HIP_DEVICE_COMPILE__)
#define DXV_PHASE_BEGIN() unsigned long long tPhase_ = __builtin_amdgcn_s_memrealtime(), ph_[10] = {0ull, 0ull, 0ull, 0ull, 0ull, 0ull, 0ull, 0ull, 0ull, 0ull}
#define DXV_PHASE(k) do { const unsigned long long now_ = __builtin_amdgcn_s_memrealtime(); ph_[k] += now_ - tPhase_; tPhase_ = now_; } while (0)
#define DXV_COUNT(k) do { ph_[k] += 1ull; } while (0)
#define DXV_PHASE_END() do { if (__builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u)) == 0u) { unsigned long long* slot_ = g_dxvPhase + (size_t)(blockIdx.x & (kPhaseSlots - 1u)) * 16u; \
    for (int k_ = 1; k_ < 10; ++k_) if (ph_[k_]) atomicAdd(slot_ + k_, ph_[k_]); } } while (0)
#else
#define DXV_PHASE_BEGIN() do { } while (0)
#define DXV_PHASE(k) do { } while (0)
#define DXV_COUNT(k) do { } while (0)
#define DXV_PHASE_END() do { } while (0)
#endif
// closest hit of the reference rule through the lists
// Two steps like the postponed-leaf walks: scanning entries is short and cheap, the triangle step is
// long, so the triangles an entry scan selects are queued in the thread's LDS column (cap entries)
// and tested when some lane's queue is full or every lane has finished scanning -- all lanes with
// work test together.
// ABL (timing-only builds, tools/ablate.py; 0 in every shipped path): 8 = stop before the texel lookup, 1 = stop after it,
// 2 = scan the entries but test no triangle, 16 = the scan's loads wave-uniform (with 2: 18), 32 / 64 = two / four more loads per scan
// round with their results unused: what one of the scan's load instructions costs
// (split at the ray's first step: the work-queue kernel makes that step for all 64 lanes of a brick at once and collects the brick
// it asked for in advance behind it -- k_voxelize_queue, voxelize_lists.hip)
// HITLDS: the closest hit's V, W, det and index live in column words cap .. cap + 3 (leaf_reference_deferred_lds); best.t and best.leaf are
// all of `best` that is meaningful then (best.leaf == -1: miss), bestDet is untouched.
// HITLDS 2: nothing but best.t and best.leaf is kept at all (leaf_reference_min, shade_reference_again).
// STARTS: what dm_ray_start<STARTS> read for `start` -- 2 (or 3 with start cells in the view): a START cell, whose scan begins by
// dm_start_cell_begin (no hint steps; the words where the hints were are the start word); else the canonical cell and start.startWord.
template <class Stack, int ABL = 0, int HITLDS = 0, int STARTS = 1>
DXV_HD void trace_reference_dm_from(Ray& r, const DirMapView& dm, const DirRayStart& start, const TriPos* tris, const Stack& stk, int cap, Hit& best,
                                    float& bestDet)
{
    best.t = kTMax; best.b1 = 0.0f; best.b2 = 0.0f; best.k = 0xffffffffu; best.leaf = -1;
    if (ABL & 8) return;
    DXV_PHASE_BEGIN();
    const DirCell cell = start.cell;
    const uint32_t cx = start.cx, cy = start.cy;
    const float rho = start.rho, near = start.near;
    // entries wholly nearer the centre than the ray's start (r1 < near: t < 0) come first: skip them --
    // all of them at once for a ray that starts beyond the texel's last triangle
    uint32_t end = cell.begin + cell.count;
    uint32_t i = cell.begin, hi = end;
    if (!start.live) i = hi;
    if (ABL & 1) { if (i == 0xffffffffu) best.k = 0u; return; }
    if (dm_reads_start_cells<dm_starts_form(STARTS)>(dm)) i = dm_start_cell_begin(cell, dm.entries, start.live, near);
    else {
        if (hi - i > 8u) {                                                  // the first two steps of the search from the texel's own words
            const uint32_t mid = i + ((hi - i) >> 1);
            const bool right = half_bits_to_float(cell.q2) < near;
            const float q = half_bits_to_float(right ? cell.q3 : cell.q1);
            if (right) i = mid + 1u; else hi = mid;
            if (hi - i > 8u) {
                const uint32_t mid2 = i + ((hi - i) >> 1);
                if (q < near) i = mid2 + 1u; else hi = mid2;
            }
        }
        while (hi - i > 8u) {
            const uint32_t mid = i + ((hi - i) >> 1);
            if (dm_entry_r1(dm.entries[mid]) < near) i = mid + 1u; else hi = mid;
        }
        // ... and the start table moves the scan's first entry later, never earlier (hints and search name positions in the whole
        // list and run as before; a ray that is not live stays at the end: the table's start never lies behind it)
        {
            const uint32_t from = cell.begin + dm_start_offset(start.startWord, cell.count, cell.r1max, near);
            if (from > i) i = from;
        }
    }
    DXV_PHASE(1);
    int qn = 0;
    bestDet = 1.0f;                                                     // divisor of the closest hit's barycentrics (the caller's finish_hit)
    const float step = dm_stop_step(half_bits_to_float(cell.thick));
    DirRayLocal loc = dm_ray_local(cx, cy);
    float bound = (rho + best.t) * 1.001f + 1e-4f;                      // how far out an entry may start and still matter: behind the closest hit so far
    uint32_t rc = dm_radial_word(near, bound);                          // radial cut: r1 >= near, r0 not beyond `bound`
    for (;;) {
        bool coop = false;                                                  // this round was a cooperative one (wave-uniform; the host: never)
#if defined(__HIP_DEVICE_COMPILE__)
        // A LONG list scanned by a LONE lane: a brick is as long as its longest list (a ray that finds no hit reads its texel's list to
        // the end: hundreds of entries in a deep fold of a real mesh, four per round, while the wave's other lanes have long
        // finished: 40 - 80 us against a median brick of 10, and a short launch cannot end before its longest brick).  When at most
        // kDmCoopLanes lanes are still scanning and the first of them has kDmCoopMin entries or more ahead, the WHOLE wave scans that
        // lane's list, one entry per lane and round (one coalesced kilobyte), with that ray's words broadcast through scalar
        // registers; what passes goes into the ray's own queue, as if it had scanned alone.  Same entries, same integer test, same
        // stop rule -- entries are only LOOKED AT in another order, and the closest hit does not depend on the order of tests.
        {
            const uint64_t sm = __builtin_amdgcn_ballot_w64(i < end);
            if (dm.coop && sm != 0ull && __builtin_popcountll(sm) <= (int)kDmCoopLanes) {
                const int L = __builtin_ctzll(sm);
                const uint32_t iL = (uint32_t)__builtin_amdgcn_readlane((int)i, L), endL = (uint32_t)__builtin_amdgcn_readlane((int)end, L);
                if (endL - iL >= kDmCoopMin) {
                    const DirRayLocal locL{(uint32_t)__builtin_amdgcn_readlane((int)loc.q, L), (uint32_t)__builtin_amdgcn_readlane((int)loc.p, L)};
                    const uint32_t rcL = (uint32_t)__builtin_amdgcn_readlane((int)rc, L);
                    const float stepL = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, step), L));
                    const float boundL = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, bound), L));
                    // (lanes of this wave that take part: a brick at the grid's end has left some behind)
                    const uint64_t act = __builtin_amdgcn_ballot_w64(true);
                    const uint32_t lane = __builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u));
                    const uint32_t rank = (uint32_t)__builtin_popcountll(act & ((1ull << lane) - 1ull)), width = (uint32_t)__builtin_popcountll(act);
                    const uint32_t at = iL + rank;
                    const bool have = at < endL;
                    const DirEntry e = dm.entries[have ? at : endL - 1u];
                    const uint64_t stop = __builtin_amdgcn_ballot_w64(have && dm_stop_radius(e, stepL) > boundL);
                    // the first entry (in list order) at which a lone scan would have stopped: nothing from there on matters
                    uint32_t stopRank = 64u;
                    if (stop) stopRank = (uint32_t)__builtin_popcountll(act & ((1ull << __builtin_ctzll(stop)) - 1ull));
                    uint64_t pm = __builtin_amdgcn_ballot_w64(have && rank < stopRank && dm_local_pass(e, locL, rcL));
                    int qnL = __builtin_amdgcn_readlane(qn, L);
                    const uint32_t triE = dm_entry_tri(e);
                    uint32_t next = stop ? endL : (iL + width < endL ? iL + width : endL);
                    while (pm) {
                        const int src = __builtin_ctzll(pm);
                        if (2 * (qnL + 1) > cap) {                           // the ray's queue is full: go on behind the last entry taken
                            next = iL + (uint32_t)__builtin_popcountll(act & ((1ull << src) - 1ull));
                            break;
                        }
                        pm &= pm - 1ull;
                        const int32_t t = __builtin_amdgcn_readlane((int)triE, src), rr = __builtin_amdgcn_readlane((int)e.rr, src);
                        if ((int)lane == L) { stk.put(2 * qn, t); stk.put(2 * qn + 1, rr); ++qn; }
                        ++qnL;
                    }
                    if ((int)lane == L) i = next;
                    coop = true;                                            // (the ray's queue may now hold up to `cap` words: no lane scans on its own in this round)
                }
            }
        }
#endif
        // four entries per round, all four loads in flight before the first is looked at (two per round:
        // +13 % on the 1 M-triangle scene, one: +40 %).  One address, four offsets: entries behind the end of the list are
        // loaded and not looked at (the next texel's, or the three spare ones behind the last list).
        if (!coop && i < end) {
            const uint32_t last = end - 1u;
            // (the third and fourth load are skipped when no lane of the wave has that many entries left:
            // -5 % on the 1 M-triangle scene; voting on the second one as well: +7 %)
            const bool wide = wave_any(i + 2u <= last);
            const DirEntry* p = dm.entries + i;
#if defined(DXV_ABLATE) && defined(__HIP_DEVICE_COMPILE__)
            // (timing only, 16: every lane loads the FIRST active lane's entries -- one line access per load instead of one per
            // lane, instruction count unchanged: what the launch would gain if the scan's loads were wave-uniform)
            if (ABL & 16) p = dm.entries + __builtin_amdgcn_readfirstlane(i);
#endif
            const DirEntry e0 = p[0], e1 = p[1];
            DirEntry e2, e3;
            if (wide && i + 2u <= last) { e2 = p[2]; e3 = p[3]; }       // (lanes whose list ends here issue no access for what they would not look at)
#if defined(DXV_ABLATE) && defined(__HIP_DEVICE_COMPILE__)
            // (timing only, 32 / 64: two / four MORE 16-byte loads per round, of the entries the next round loads anyway, results
            // unused: the slope is what one of the scan's load instructions costs)
            if (ABL & (32 | 64)) {
                const DirEntry x0 = p[4], x1 = p[5];
                asm volatile("" :: "v"(x0.box), "v"(x1.box));
                if (ABL & 64) { const DirEntry x2 = p[6], x3 = p[7]; asm volatile("" :: "v"(x2.box), "v"(x3.box)); }
            }
#endif
            // The list is sorted by far radius and every entry knows (in 63rds of the texel's thickest entry) how far behind
            // its far radius the earliest start of any LATER entry lies: once that point is beyond the closest hit so far,
            // this entry and everything behind it start beyond the hit.  (Surface meshes have short lists and gain
            // little; in a deep soup a ray stops after the first few of hundreds of entries.)
            if (dm_stop_radius(e0, step) > bound) i = end;
            else {
                // (a queued item is two words: the triangle, and the entry's radial word for the second look below)
                if (dm_local_pass(e0, loc, rc)) { stk.put(2 * qn, (int32_t)dm_entry_tri(e0)); stk.put(2 * qn + 1, (int32_t)e0.rr); ++qn; }
                if (i + 1u <= last && dm_local_pass(e1, loc, rc)) { stk.put(2 * qn, (int32_t)dm_entry_tri(e1)); stk.put(2 * qn + 1, (int32_t)e1.rr); ++qn; }
                if (wide) {
                    if (i + 2u <= last && dm_local_pass(e2, loc, rc)) { stk.put(2 * qn, (int32_t)dm_entry_tri(e2)); stk.put(2 * qn + 1, (int32_t)e2.rr); ++qn; }
                    if (i + 3u <= last && dm_local_pass(e3, loc, rc)) { stk.put(2 * qn, (int32_t)dm_entry_tri(e3)); stk.put(2 * qn + 1, (int32_t)e3.rr); ++qn; }
                }
                i += 4u;
            }
        }
        const bool scanning = wave_any(i < end);
        DXV_PHASE(2); DXV_COUNT(7);
        if (scanning && !wave_any(2 * (qn + 4) > cap)) continue;
        DXV_COUNT(9);
        if (ABL & 2) { if (qn > 100) best.k = 0u; }
        else {
            // direction, 1 / d, -o / d (hlsl:52 and the slab constants): only now, after the scan of the short lists of a
            // surface mesh is over -- two waves in five never get here, and the scan runs with a dozen registers less
            finish_ray_reference(r, rho);                               // (|o| is the ray's start radius: the same expression, dm_ray_point)
            ray_shear_finished(r);                                      // (here, not at the first triangle: the direction's registers are free through the tests)
            DXV_PHASE(3);
            // Every lane takes its queued triangles in turn, but looks at an item's near radius once more first: what starts
            // beyond a hit found since it was queued is dropped unfetched, so a round is one triangle for every lane that
            // still has a live item (the most loaded lane of a wave decides how many rounds there are).
            int k = 0;
            for (;;) {
                while (k < qn && (((uint32_t)stk.get(2 * k + 1) - rc) & 0x00008000u) == 0u) ++k;      // r0 beyond the closest hit so far
                if (!wave_any(k < qn)) break;
                if (k < qn) {
                    if (HITLDS == 2) leaf_reference_min(r, tris, stk.get(2 * k), best.t, best.leaf);
                    else if (HITLDS == 1) leaf_reference_deferred_lds(r, tris, stk.get(2 * k), best.t, best.leaf, stk, cap);
                    else leaf_reference_deferred(r, tris, stk.get(2 * k), best, bestDet);
                    bound = (rho + best.t) * 1.001f + 1e-4f;
                    rc = dm_radial_word(near, bound);
                    ++k;
                }
                DXV_COUNT(8);
            }
            DXV_PHASE(4);
        }
        qn = 0;
        if (!scanning) break;
    }
    DXV_PHASE_END();
}

// Row lists of the parity rule (parity_lists.hip): the texels of the R x R grid over the (y, z) plane that a triangle's padded box --
// the box parity_row_setup tests a row against -- reaches; a row's texel is (dm_texel(oy), dm_texel(oz)), monotone in the
// coordinate, so a row inside the box lies in a texel of the rectangle.
DXV_HD void pl_rect(const TriPos& tp, uint32_t R, uint32_t& j0, uint32_t& j1, uint32_t& k0, uint32_t& k1)
{
    float lo[3], hi[3];
    tri_box(tp.v0, tp.v1, tp.v2, lo, hi);
    j0 = dm_texel(lo[1], R); j1 = dm_texel(hi[1], R); k0 = dm_texel(lo[2], R); k1 = dm_texel(hi[2], R);
}

template <class Stack, int ABL = 0>
DXV_HD void trace_reference_dm(Ray& r, const DirMapView& dm, const TriPos* tris, const Stack& stk, int cap, Hit& best, float& bestDet)
{
    if (ABL & 8) { best.t = kTMax; best.b1 = 0.0f; best.b2 = 0.0f; best.k = 0xffffffffu; best.leaf = -1; return; }
    // (start cells where the view has them -- a launch that reads the table --, else the canonical cell and the table's word, if any)
    const DirRayStart start = dm_ray_start<3>(r.ox, r.oy, r.oz, dm);
    trace_reference_dm_from<Stack, ABL, 0, 3>(r, dm, start, tris, stk, cap, best, bestDet);
}

template <class Stack, int ABL>
DXV_HD void trace_reference_lists(Ray& r, const SceneView& sc, const Stack& stk, int cap, Hit& best, float& bestDet)
{
    const DirMapView dm{static_cast<const DirCell*>(sc.dmCells), static_cast<const DirEntry*>(sc.dmEntries), sc.dmR, sc.dmCoop, sc.dmStarts, static_cast<const DirCell*>(sc.dmStartCells)};
    trace_reference_dm<Stack, ABL>(r, dm, sc.triPos, stk, cap, best, bestDet);
}

} // namespace dxv
