// pad_check.cpp -- TEST-ONLY: the lateral bound of the lists' builder (dxv_dirmap.h: dm_lateral_pad) against the triangle step itself.
// One translation unit with filter_check.cpp (and through it start_table_check.cpp and hostcheck.cpp): the host scene and the product's
// own __host__ __device__ code as they stand, plus:
//   pc_family        seeded families of triangles, a few thousand rays at and around every edge and vertex of each: a ray that
//                    leaf_reference_min ACCEPTS must find the triangle in its texel (dm_rect, dm_texel_outside) and pass the entry
//                    dm_local_entry builds there (dm_local_pass) -- with a factor on the record's pad on the test's side only
//   pc_monotone      per record: the narrow pad against the 2^-15 pad -- pad, texel rectangle, texel set, and per texel box and edge
//                    over all 128 x 128 cells
//   pc_dirmap_build  hc_dirmap_build with option lateralpad as an argument
// Never linked into libdxv.so.  With -DPAD_CHECK_MAIN: a stand-alone program (one small run of every family; for sanitizer builds).
#include "filter_check.cpp"

namespace {

struct PcRng {
    uint64_t s;
    uint64_t next() { uint64_t z = (s += 0x9e3779b97f4a7c15ull); z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull; z = (z ^ (z >> 27)) * 0x94d049bb133111ebull; return z ^ (z >> 31); }
    double uni() { return (double)(next() >> 11) * (1.0 / 9007199254740992.0); }
    double uni(double a, double b) { return a + (b - a) * uni(); }
    double log10uni(double a, double b) { return __builtin_pow(10.0, uni(a, b)); }
    uint32_t below(uint32_t n) { return (uint32_t)(next() % n); }
};

struct V3 { double x, y, z; };
inline V3 operator+(V3 a, V3 b) { return {a.x + b.x, a.y + b.y, a.z + b.z}; }
inline V3 operator-(V3 a, V3 b) { return {a.x - b.x, a.y - b.y, a.z - b.z}; }
inline V3 operator*(double s, V3 a) { return {s * a.x, s * a.y, s * a.z}; }
inline double dot(V3 a, V3 b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
inline V3 cross(V3 a, V3 b) { return {a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x}; }
inline double len(V3 a) { return __builtin_sqrt(dot(a, a)); }
inline V3 unit(V3 a) { const double l = len(a); return l > 0.0 ? (1.0 / l) * a : V3{1.0, 0.0, 0.0}; }
inline double clamp1(double x) { return x < -1.0 ? -1.0 : x > 1.0 ? 1.0 : x; }
inline V3 clampCube(V3 a) { return {clamp1(a.x), clamp1(a.y), clamp1(a.z)}; }
V3 randDir(PcRng& g)
{
    for (;;) {
        const V3 v{g.uni(-1, 1), g.uni(-1, 1), g.uni(-1, 1)};
        const double l = len(v);
        if (l > 0.05 && l <= 1.0) return (1.0 / l) * v;
    }
}
V3 anyPerp(V3 a, PcRng& g) { for (;;) { const V3 c = cross(a, randDir(g)); if (len(c) > 0.1) return unit(c); } }
// a point of the cube at depth 0.05 .. 1.0 along its dominant axis (radius up to 1.7)
V3 randCentre(PcRng& g, double lo = 0.05)
{
    V3 c{g.uni(-1, 1), g.uni(-1, 1), g.uni(-1, 1)};
    const double m = __builtin_fmax(__builtin_fabs(c.x), __builtin_fmax(__builtin_fabs(c.y), __builtin_fabs(c.z)));
    const double want = g.uni() < 0.3 ? g.log10uni(__builtin_log10(lo), 0.0) : g.uni(lo, 1.0);
    return (want / (m > 1e-9 ? m : 1.0)) * c;
}

enum { kWell = 0, kSliver, kGrazing, kSnapped, kNearPlane, kSpanning, kUnit, kFamilies };

// one triangle of a family (double; rounded to fp32 by the caller)
void makeTriangle(int family, PcRng& g, V3 v[3])
{
    const double delta = (double)kDmDelta;
    switch (family) {
    default:
    case kWell: {
        const V3 c = randCentre(g);
        const double s = g.log10uni(-3.0, -0.3);
        for (int i = 0; i < 3; ++i) v[i] = clampCube(c + s * V3{g.uni(-1, 1), g.uni(-1, 1), g.uni(-1, 1)});
        break;
    }
    case kSliver: {                                                     // altitude 1e-8 .. 1e-3 of the longest edge
        const V3 a = randCentre(g), d = randDir(g);
        const double l = g.log10uni(-2.0, 0.0);
        const V3 b = clampCube(a + l * d);
        const V3 n = anyPerp(unit(b - a), g);
        v[0] = a; v[1] = b; v[2] = clampCube(a + g.uni(g.uni() < 0.3 ? -0.2 : 0.0, 1.0) * (b - a) + (g.log10uni(-8.0, -3.0) * len(b - a)) * n);
        break;
    }
    case kGrazing: {                                                    // the normal within 1e-6 .. 1e-2 of 90 degrees of the rays
        const V3 c = randCentre(g, 0.2), r = unit(c), t1 = anyPerp(r, g), t2 = cross(r, t1);
        const double eps = g.log10uni(-6.0, -2.0) * (g.uni() < 0.5 ? 1.0 : -1.0), s = g.log10uni(-2.5, -0.5);
        const V3 e1 = __builtin_cos(eps) * r - __builtin_sin(eps) * t2;  // in the plane, nearly along the rays
        for (int i = 0; i < 3; ++i) v[i] = c + s * (g.uni(-1, 1) * e1 + g.uni(-1, 1) * t1);
        bool in = true;
        for (int i = 0; i < 3; ++i) in = in && __builtin_fabs(v[i].x) <= 1.0 && __builtin_fabs(v[i].y) <= 1.0 && __builtin_fabs(v[i].z) <= 1.0;
        if (!in) for (int i = 0; i < 3; ++i) v[i] = 0.5 * v[i];         // (scaling about the centre keeps the plane through the rays)
        break;
    }
    case kSnapped: {                                                    // vertices on a voxel lattice, or on texel and cell borders of a map
        const V3 c = randCentre(g);
        const double s = g.log10uni(-2.0, -0.5);
        const uint32_t N = 16u << g.below(6);
        const bool lattice = g.uni() < 0.5, centres = g.uni() < 0.5;
        const uint32_t R = 16u << g.below(6);
        for (int i = 0; i < 3; ++i) {
            V3 p = clampCube(c + s * V3{g.uni(-1, 1), g.uni(-1, 1), g.uni(-1, 1)});
            if (lattice) {
                const double h = 2.0 / N, o = centres ? 0.5 * h : 0.0;
                p = {__builtin_floor((p.x + 1.0) / h) * h + o - 1.0, __builtin_floor((p.y + 1.0) / h) * h + o - 1.0, __builtin_floor((p.z + 1.0) / h) * h + o - 1.0};
            } else {                                                    // u, v on borders of cells (1 / 128 of a texel) at the vertex' own depth
                double q[3] = {p.x, p.y, p.z};
                int a = 0;
                for (int k = 1; k < 3; ++k) if (__builtin_fabs(q[k]) > __builtin_fabs(q[a])) a = k;
                const double d = __builtin_fabs(q[a]), cell = 2.0 / (R * (g.uni() < 0.5 ? 1.0 : 128.0));
                for (int k = 0; k < 3; ++k) if (k != a) q[k] = (__builtin_floor((q[k] / d + 1.0) / cell) * cell - 1.0) * d;
                p = {q[0], q[1], q[2]};
            }
            v[i] = clampCube(p);
        }
        break;
    }
    case kNearPlane: {                                                  // a vertex within 64 delta (and a little beyond) of a face plane or of the centre
        const V3 c = randCentre(g, 0.1);
        const double s = g.log10uni(-2.0, -0.3);
        for (int i = 0; i < 3; ++i) v[i] = clampCube(c + s * V3{g.uni(-1, 1), g.uni(-1, 1), g.uni(-1, 1)});
        double* q = &v[g.below(3)].x;
        const double small = g.uni(-128.0, 128.0) * delta;
        if (g.uni() < 0.3) { q[0] = g.uni(-128.0, 128.0) * delta; q[1] = g.uni(-128.0, 128.0) * delta; q[2] = small; }
        else q[g.below(3)] = small;
        break;
    }
    case kSpanning: {                                                   // across two and three faces of the map
        const V3 c = randCentre(g, 0.2);
        const double s = g.uni(0.3, 1.5);
        for (int i = 0; i < 3; ++i) v[i] = clampCube(c + s * V3{g.uni(-1, 1), g.uni(-1, 1), g.uni(-1, 1)});
        break;
    }
    case kUnit: {                                                       // coordinates at +-1
        const V3 c = randCentre(g, 0.5);
        const double s = g.log10uni(-2.0, 0.0);
        for (int i = 0; i < 3; ++i) {
            v[i] = clampCube(c + s * V3{g.uni(-1, 1), g.uni(-1, 1), g.uni(-1, 1)});
            double* q = &v[i].x;
            if (g.uni() < 0.6) { const uint32_t k = g.below(3); q[k] = q[k] < 0.0 ? -1.0 : 1.0; }
        }
        break;
    }
    }
    if (g.uni() < 0.5) { const V3 t = v[1]; v[1] = v[2]; v[2] = t; }    // both orientations
}

struct PcRecords { DirRecord rec[6]; };
// the six records of a triangle as the list build makes them (lateral: option lateralpad)
PcRecords recordsOf(const TriPos& tp, bool lateral)
{
    PcRecords r;
    for (uint32_t f = 0; f < 6u; ++f) r.rec[f] = dm_record(tp, f, lateral);
    return r;
}
// the record with `factor` on its pad, on the test's side: the edges move with rec.pad; the box of a record with a bound of its own follows
// (dm_record_box), the box of any other record is the 2^-15 pad's and is taken in by the same amount here.  factor 1: the record as it is.
DirRecord scaled(const DirRecord& rec, double factor)
{
    if (factor == 1.0 || !(rec.hasTri & 1u)) return rec;
    DirRecord r = rec;
    r.pad = (float)(rec.pad * factor);
    if (!(rec.hasTri & kDmRecLateral) && rec.u0 <= rec.u1) {
        const float s = (float)((1.0 - factor) * rec.pad);
        if (r.u0 + s < r.u1 - s) { r.u0 += s; r.u1 -= s; }
        if (r.v0 + s < r.v1 - s) { r.v0 += s; r.v1 -= s; }
    }
    return r;
}

struct PcCount { uint64_t rays = 0, accepted = 0, violations = 0, notInRect = 0, texelOutside = 0, entryFails = 0, acceptedLateral = 0; };

// one ray from origin o against triangle tp: accepted => listed (out: the counters)
void castRay(const TriPos& tp, const PcRecords& recs, double factor, uint32_t R, float ox, float oy, float oz, PcCount& c)
{
    if (!(ox != 0.0f || oy != 0.0f || oz != 0.0f)) return;
    if (!(__builtin_fabsf(ox) <= 1.0f && __builtin_fabsf(oy) <= 1.0f && __builtin_fabsf(oz) <= 1.0f)) return;     // voxel centres lie in the cube
    ++c.rays;
    Ray r;
    r.ox = ox; r.oy = oy; r.oz = oz;
    uint32_t face;
    float u, v, rho;
    dm_ray_point(ox, oy, oz, face, u, v, rho);
    if (!(rho > 4e-4f)) return;                                         // (a ray starts at least half a voxel diagonal from the centre)
    finish_ray_reference(r, rho);
    ray_shear_finished(r);
    float t = kTMax;
    int32_t leaf = -1;
    leaf_reference_min(r, &tp, 0, t, leaf);
    if (leaf == -1) return;
    ++c.accepted;
    DirRecord rec = scaled(recs.rec[face], factor);
    if (rec.hasTri & kDmRecLateral) ++c.acceptedLateral;
    uint32_t ti, tj, cx, cy, i0, i1, j0, j1;
    dm_local(u, R, ti, cx); dm_local(v, R, tj, cy);
    if (!dm_rect(rec, R, i0, i1, j0, j1) || ti < i0 || ti > i1 || tj < j0 || tj > j1) { ++c.violations; ++c.notInRect; return; }
    const uint32_t texels = (i1 - i0 + 1u) * (j1 - j0 + 1u);
    dm_record_on_map(rec, texels);
    if (dm_texel_outside(dm_texel_test(rec, texels), R, ti, tj)) { ++c.violations; ++c.texelOutside; return; }
    const DirEntry e = dm_local_entry(rec, R, ti, tj, 0u);
    // the ray's radial cut: as the scan begins (no hit yet) -- and, for a record with a bound of its own, as it is once this very hit is the
    // closest, the strictest cut the entry can meet (its per-texel range is made with the record's pad).  Not asked of the other records: a
    // sliver's computed t is a quotient of two rounding errors and can lie percent in front of the sliver (a ray of the sliver family,
    // seed 20261020, found with t = 0.3867 from rho = 0.5136 a triangle whose nearest point is at 0.9257) -- their radial margins are not
    // this check's subject
    const float near = rho * 0.999f, bound = ((rec.hasTri & kDmRecLateral) ? rho + t : rho + kTMax) * 1.001f + 1e-4f;
    if (!dm_local_pass(e, dm_ray_local(cx, cy), dm_radial_word(near, bound))) { ++c.violations; ++c.entryFails; }
}

TriPos toTriPos(const V3 v[3])
{
    TriPos tp;
    tp.v0 = {(float)v[0].x, (float)v[0].y, (float)v[0].z, 0.0f}; tp.v1 = {(float)v[1].x, (float)v[1].y, (float)v[1].z, 0.0f};
    tp.v2 = {(float)v[2].x, (float)v[2].y, (float)v[2].z, 0.0f};
    return tp;
}

// The rays of one triangle: targets on, inside and up to 1.5 x the 2^-15 pad outside every edge and beyond every vertex (in the plane and
// off it), each seen from several start radii in front of it; and for grids 16 .. 512 the voxel centres nearest the lines through the
// vertices and the edges' thirds, slice by slice.
void castTriangle(const TriPos& tp, const PcRecords& recs, double factor, PcRng& g, uint32_t raysPerEdge, bool voxels, PcCount& c)
{
    const V3 P[3] = {{tp.v0.x, tp.v0.y, tp.v0.z}, {tp.v1.x, tp.v1.y, tp.v1.z}, {tp.v2.x, tp.v2.y, tp.v2.z}};
    const V3 n = unit(cross(P[1] - P[0], P[2] - P[0]));
    const double delta = (double)kDmDelta;
    static const uint32_t kMaps[5] = {16u, 64u, 256u, 512u, 2048u};
    for (int k = 0; k < 3; ++k) {
        const V3 A = P[k], B = P[(k + 1) % 3], C = P[(k + 2) % 3];
        const V3 e = B - A;
        V3 out = cross(e, n);                                           // in the plane, away from the third vertex
        if (dot(out, C - A) > 0.0) out = -1.0 * out;
        out = unit(out);
        for (uint32_t q = 0; q < raysPerEdge; ++q) {
            const double mode = g.uni();
            // along the edge: inside it, at its ends, and beyond them by up to 1.5 x the pad (or 30 % of its length)
            double s = mode < 0.5 ? g.uni(0.0, 1.0) : mode < 0.7 ? (g.uni() < 0.5 ? 0.0 : 1.0) : g.uni(-0.3, 1.3);
            V3 T = A + s * e;
            if (mode >= 0.7 && mode < 0.85 && len(e) > 0.0) T = (s < 0.5 ? A : B) + ((s < 0.5 ? -1.0 : 1.0) * g.uni(0.0, 1.5) * 2.25 * delta * len(T) / len(e)) * e;
            // sideways: the depth the pad is meant at is the target's own, so 2.25 delta |T| is about the pad in face coordinates there
            const double w = 2.25 * delta * (len(T) > 0.05 ? len(T) : 0.05);
            const double kind = g.uni();
            const double off = kind < 0.35 ? g.uni(-1.5, 1.5) * w : kind < 0.7 ? g.uni(-0.15, 0.15) * w : kind < 0.85 ? g.uni(-1.0, 1.0) * 1e-7 : 0.0;
            T = T + off * out;
            if (g.uni() < 0.3) T = T + (g.uni(-1.5, 1.5) * w) * n;          // off the plane: what moves a grazing triangle's projection
            const uint32_t R = kMaps[g.below(5)];
            // start radii in front of the target: far, near, and a hair in front
            const double fr[4] = {g.uni(0.05, 0.6), g.uni(0.6, 0.98), 1.0 - g.log10uni(-5.0, -2.0), 1.0 - g.log10uni(-7.0, -5.0)};
            for (int a = 0; a < 4; ++a) castRay(tp, recs, factor, R, (float)(fr[a] * T.x), (float)(fr[a] * T.y), (float)(fr[a] * T.z), c);
        }
    }
    if (!voxels) return;
    // voxel centres: for every grid, every slice of the dominant axis between the centre and the target, the voxel nearest the line
    // from the centre to the target (vertices, and the thirds of the edges)
    for (int k = 0; k < 3; ++k)
        for (int h = 0; h < 3; ++h) {
            const V3 T = P[k] + (h / 3.0) * (P[(k + 1) % 3] - P[k]);
            const double q[3] = {T.x, T.y, T.z};
            int a = 0;
            for (int m = 1; m < 3; ++m) if (__builtin_fabs(q[m]) > __builtin_fabs(q[a])) a = m;
            if (!(__builtin_fabs(q[a]) > 1e-3)) continue;
            for (uint32_t N = 16u; N <= 512u; N *= 2u) {
                const uint32_t R = kMaps[g.below(5)];
                for (uint32_t s = 0; s < N / 2u; ++s) {
                    const double xa = (s + 0.5) * 2.0 / N;                 // |coordinate| of the slice's voxel centres
                    if (xa > __builtin_fabs(q[a])) break;
                    const double lam = xa / __builtin_fabs(q[a]);
                    uint32_t idx[3];
                    for (int m = 0; m < 3; ++m) {
                        const double x = lam * q[m];
                        const double f = __builtin_floor((x + 1.0) * 0.5 * N);
                        idx[m] = f < 0.0 ? 0u : f >= (double)N ? N - 1u : (uint32_t)f;
                    }
                    float ox, oy, oz;
                    ray_origin(N, idx[0], N - 1u - idx[1], idx[2], ox, oy, oz);    // (y falls with iy)
                    castRay(tp, recs, factor, R, ox, oy, oz, c);
                }
            }
        }
}

} // namespace

extern "C" {

// One family: `count` triangles from `seed`, raysPerEdge x 4 rays around each edge, voxel-centre rays for every `voxelEvery`-th triangle
// (0: none).  lateral: the records as option lateralpad makes them; factor: on the records' pad, the test's side only.
// out[0] rays, [1] accepted, [2] violations, [3] ray's texel outside dm_rect, [4] dm_texel_outside, [5] dm_local_pass fails,
// [6] accepted rays whose record has a bound of its own, [7] (triangle, face) records with a projected triangle, [8] of those with a bound of their own
__attribute__((visibility("default"))) void pc_family(int family, uint64_t seed, uint32_t count, uint32_t raysPerEdge, uint32_t voxelEvery, int lateral,
                                                      double factor, uint64_t* out)
{
    uint64_t o[9] = {0};
#pragma omp parallel for schedule(dynamic, 16) reduction(+ : o[:9])
    for (int64_t i = 0; i < (int64_t)count; ++i) {
        PcRng g{seed * 0x100000001b3ull + (uint64_t)i * 0x9e3779b97f4a7c15ull + (uint64_t)family};
        V3 v[3];
        makeTriangle(family, g, v);
        const TriPos tp = toTriPos(v);
        const PcRecords recs = recordsOf(tp, lateral != 0);
        for (int f = 0; f < 6; ++f) if (recs.rec[f].hasTri & 1u) { ++o[7]; if (recs.rec[f].hasTri & kDmRecLateral) ++o[8]; }
        PcCount c;
        castTriangle(tp, recs, factor, g, raysPerEdge, voxelEvery && i % voxelEvery == 0, c);
        o[0] += c.rays; o[1] += c.accepted; o[2] += c.violations; o[3] += c.notInRect; o[4] += c.texelOutside; o[5] += c.entryFails; o[6] += c.acceptedLateral;
    }
    for (int k = 0; k < 9; ++k) out[k] = o[k];
}

// Monotonicity of one triangle's records on an R-texel map: the record made with the bound against the record made without.
// out[0] records compared (a footprint on the map), [1] with a bound of their own, [2] pad larger, [3] texel rectangle not inside,
// [4] texels listed with the bound and not without, [5] texels whose box is not inside, [6] texels whose edge passes a cell the wide
// one fails (all 128 x 128 cells), [7] texels compared cell by cell, [8] texels listed without the bound, [9] with it
static void monotoneOne(const TriPos& tp, uint32_t R, uint64_t* o)
{
    for (uint32_t f = 0; f < 6u; ++f) {
        DirRecord wide = dm_record(tp, f, false), own = dm_record(tp, f, true);
        uint32_t a0, a1, b0, b1, i0, i1, j0, j1;
        const bool seenWide = dm_rect(wide, R, a0, a1, b0, b1), seenOwn = dm_rect(own, R, i0, i1, j0, j1);
        if (!seenWide && !seenOwn) continue;
        ++o[0];
        if (own.hasTri & kDmRecLateral) ++o[1];
        if (!(own.pad <= wide.pad)) ++o[2];
        if (seenOwn && (!seenWide || i0 < a0 || i1 > a1 || j0 < b0 || j1 > b1)) { ++o[3]; continue; }
        if (!seenOwn) continue;
        const uint32_t texWide = (a1 - a0 + 1u) * (b1 - b0 + 1u), texOwn = (i1 - i0 + 1u) * (j1 - j0 + 1u);
        dm_record_on_map(wide, texWide); dm_record_on_map(own, texOwn);
        const DirTexelTest tw = dm_texel_test(wide, texWide), to = dm_texel_test(own, texOwn);
        for (uint32_t j = b0; j <= b1; ++j) for (uint32_t i = a0; i <= a1; ++i) if (!dm_texel_outside(tw, R, i, j)) ++o[8];
        if (texOwn > 4096u) continue;                                   // (a face-filling footprint: rectangle and pad compared, not every texel)
        for (uint32_t j = j0; j <= j1; ++j)
            for (uint32_t i = i0; i <= i1; ++i) {
                if (dm_texel_outside(to, R, i, j)) continue;
                ++o[9];
                if (dm_texel_outside(tw, R, i, j)) { ++o[4]; continue; }
                if (!(own.hasTri & kDmRecLateral)) continue;            // (the same record bit for bit: nothing to compare)
                const DirEntry ew = dm_local_entry(wide, R, i, j, 0u), eo = dm_local_entry(own, R, i, j, 0u);
                ++o[7];
                bool boxIn = true;
                for (int k = 0; k < 4; ++k) boxIn = boxIn && ((eo.box >> (8 * k)) & 0xffu) >= ((ew.box >> (8 * k)) & 0xffu);   // (each byte a lower limit)
                if (!boxIn) ++o[5];
                bool edgeIn = true;
                for (uint32_t y = 0; y < kDmCells && edgeIn; ++y)
                    for (uint32_t x = 0; x < kDmCells; ++x) {
                        const uint32_t p = dm_ray_local(x, y).p;
                        if (dm_dot4(eo.edge, p) >= 0 && !(dm_dot4(ew.edge, p) >= 0)) { edgeIn = false; break; }
                    }
                if (!edgeIn) ++o[6];
            }
    }
}
__attribute__((visibility("default"))) void pc_monotone_family(int family, uint64_t seed, uint32_t count, uint64_t* out)
{
    uint64_t o[10] = {0};
    static const uint32_t kMaps[4] = {16u, 64u, 256u, 512u};
#pragma omp parallel for schedule(dynamic, 8) reduction(+ : o[:10])
    for (int64_t i = 0; i < (int64_t)count; ++i) {
        PcRng g{seed * 0x100000001b3ull + (uint64_t)i * 0x9e3779b97f4a7c15ull + (uint64_t)family};
        V3 v[3];
        makeTriangle(family, g, v);
        monotoneOne(toTriPos(v), kMaps[i & 3], o);
    }
    for (int k = 0; k < 10; ++k) out[k] = o[k];
}
// ... and of every triangle of a host scene
__attribute__((visibility("default"))) void pc_monotone_scene(void* p, uint32_t R, uint64_t* out)
{
    HcScene* s = static_cast<HcScene*>(p);
    uint64_t o[10] = {0};
#pragma omp parallel for schedule(dynamic, 64) reduction(+ : o[:10])
    for (int64_t t = 0; t < (int64_t)s->T; ++t) monotoneOne(s->triPos[t], R, o);
    for (int k = 0; k < 10; ++k) out[k] = o[k];
}

// hc_dirmap_build (hostcheck.cpp) with option lateralpad as an argument: the records made with (1) or without (0) the bound, everything
// behind them by hc_dirmap_build's own steps.  Returns the number of entries.
__attribute__((visibility("default"))) uint64_t pc_dirmap_build(void* p, uint32_t R, int lateral)
{
    HcScene* s = static_cast<HcScene*>(p);
    if (lateral) return hc_dirmap_build(p, R);
    // the 2^-15 pad for every record: the same build over triangles whose records are made with lateral = false.  hc_dirmap_build has
    // no such switch, so its steps are repeated here on the records made the other way.
    std::vector<uint64_t> keys;
    std::vector<DirRecord> rec((size_t)s->T * 6);
    const DirKeyLayout lay = dm_key_layout(R);
    for (int64_t t6 = 0; t6 < (int64_t)s->T * 6; ++t6) {
        const uint32_t t = (uint32_t)(t6 / 6), f = (uint32_t)(t6 % 6);
        DirRecord e = dm_record(s->triPos[t], f, false);
        uint32_t i0, i1, j0, j1;
        const bool seen = dm_rect(e, R, i0, i1, j0, j1);
        if (seen) dm_record_on_map(e, (i1 - i0 + 1u) * (j1 - j0 + 1u));
        rec[(size_t)t * 6 + f] = e;
        if (!seen) continue;
        const DirTexelTest tt = dm_texel_test(e, (i1 - i0 + 1u) * (j1 - j0 + 1u));
        for (uint32_t j = j0; j <= j1; ++j)
            for (uint32_t i = i0; i <= i1; ++i) {
                if (dm_texel_outside(tt, R, i, j)) continue;
                uint32_t r0h, r1h;
                dm_local_radial(e, R, i, j, r0h, r1h);
                keys.push_back(dm_key(lay, (f * R + j) * R + i, (uint16_t)r1h, t));
            }
    }
    std::sort(keys.begin(), keys.end());
    s->dmR = R;
    s->dmCells.assign((size_t)6 * R * R, DirCell{0, 0, 0, 0, 0, 0, 0});
    s->dmEntries.assign(keys.size() + 3, DirEntry{0, 0, 0, 0});
    for (size_t i = 0; i < keys.size(); ++i) {
        const uint32_t cell = dm_key_cell(lay, keys[i]), t = dm_key_tri(lay, keys[i]);
        const uint32_t inFace = cell % (R * R);
        s->dmEntries[i] = dm_local_entry(rec[(size_t)t * 6 + cell / (R * R)], R, inFace % R, inFace / R, t);
    }
    for (size_t i = 0; i < keys.size(); ++i) {
        const uint32_t cell = dm_key_cell(lay, keys[i]);
        if (i == 0 || dm_key_cell(lay, keys[i - 1]) != cell) s->dmCells[cell].begin = (uint32_t)i;
        if (s->dmCells[cell].count == 0xffffu) return ~0ull;
        s->dmCells[cell].count++;
        s->dmCells[cell].r1max = (uint16_t)((s->dmEntries[i].rr >> 16) & 0x7fffu);
        const uint32_t th = half_up(dm_entry_r1(s->dmEntries[i]) - dm_entry_r0(s->dmEntries[i]));
        if (th > s->dmCells[cell].thick) s->dmCells[cell].thick = (uint16_t)th;
    }
    for (DirCell& cell : s->dmCells) {
        const float step = dm_stop_step(half_bits_to_float(cell.thick));
        float smin = 3.0e38f;
        for (uint32_t k = cell.count; k-- > 0u;) {
            DirEntry& e = s->dmEntries[cell.begin + k];
            if (dm_entry_r0(e) < smin) smin = dm_entry_r0(e);
            e.tri = (e.tri & kDmTriMask) | (dm_stop_code(dm_entry_r1(e), smin, step) << kDmTriBits);
        }
        if (cell.count <= 8u) continue;
        const DirSearchHints h = dm_search_hints(cell.count);
        auto r1 = [&](uint32_t k) { return (uint16_t)((s->dmEntries[cell.begin + k].rr >> 16) & 0x7fffu); };
        cell.q2 = r1(h.m2);
        if (h.has1) cell.q1 = r1(h.m1);
        if (h.has3) cell.q3 = r1(h.m3);
    }
    return keys.size();
}

} // extern "C"

#if defined(PAD_CHECK_MAIN)
#include <cstdio>
// stand-alone: a small run of every family at factor 1 (0 violations expected) and of the monotonicity check; exit status 1 on a violation
int main()
{
    int bad = 0;
    for (int family = 0; family < kFamilies; ++family) {
        uint64_t o[9], m[10];
        pc_family(family, 20261020u, 400u, 40u, 50u, 1, 1.0, o);
        pc_monotone_family(family, 20261020u, 200u, m);
        std::printf("family %d: rays %llu accepted %llu violations %llu | records %llu pad> %llu rect %llu texels %llu box %llu edge %llu\n", family,
                    (unsigned long long)o[0], (unsigned long long)o[1], (unsigned long long)o[2], (unsigned long long)m[0], (unsigned long long)m[2],
                    (unsigned long long)m[3], (unsigned long long)m[4], (unsigned long long)m[5], (unsigned long long)m[6]);
        if (o[2] || m[2] || m[3] || m[4] || m[5] || m[6]) bad = 1;
    }
    return bad;
}
#endif
