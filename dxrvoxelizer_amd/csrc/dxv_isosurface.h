// dxv_isosurface.h -- naive Surface Nets over a float32 field of a whole N^3 grid (DESIGN.md §2 writes every operation out): one vertex in
// every lattice cell with a sign change, one quad -- two triangles -- on every lattice edge with one.  The lattice is the grid's samples
// padded by one layer (sample indices -1 .. N per axis, the padding worth one voxel P of the field's unit), so a solid that touches the
// grid's border is capped; cell c = (cx, cy, cz), each index 0 .. N, has the corners c - 1 + (dx, dy, dz), kept here as s[dx | dy << 1 |
// dz << 2].  Cells are numbered (cz (N + 1) + cy) (N + 1) + cx and handled 64 at a time along x: word (cz (N + 1) + cy) W + cx / 64 holds
// one bit per cell of the run ("has a vertex"), the exclusive sums of the words' vertices and quads give every vertex and every quad its
// place, so the mesh is in cell order whatever the scheduling.
// Everything here is __host__ __device__: isosurface.hip runs it on the GPU, tests/test_isosurface_rule.py compiles the same text for the CPU.
#pragma once
#include <math.h>
#include <stddef.h>
#include "dxv_types.h"
#include "dxv_scratch.h"

namespace dxv {

struct IsoVertex { float px, py, pz, nx, ny, nz; };                     // 24 bytes: the vertex layout of dxv_set_mesh
struct IsoCounts { uint32_t vertices, quads; };                         // of one word; after the scan: of all the words before it

constexpr uint64_t kIsoMaxCount = 0x7fffffffull;                        // vertices, and index words, of a mesh at the most

DXV_HD uint32_t iso_row_words(uint32_t N) { return (N + 1u + 63u) / 64u; }
DXV_HD size_t iso_words(uint32_t N) { return (size_t)(N + 1u) * (N + 1u) * iso_row_words(N); }

DXV_HD bool iso_inside(float v) { return v < 0.0f; }                   // (-0, +0 and NaN are outside)
DXV_HD bool iso_finite(float v) { return v - v == 0.0f; }              // (Inf - Inf and NaN - NaN are NaN)
DXV_HD uint32_t iso_popc(uint64_t v)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return (uint32_t)__popcll(v);
#else
    return (uint32_t)__builtin_popcountll(v);
#endif
}

// sample (i, j, k), each index -1 .. N: one subtraction inside the grid, one voxel outside it
DXV_HD float iso_sample(const float* field, uint32_t N, int32_t i, int32_t j, int32_t k, float iso, float P)
{
    if ((uint32_t)i >= N || (uint32_t)j >= N || (uint32_t)k >= N) return P;
    return field[((size_t)k * N + (uint32_t)j) * N + (uint32_t)i] - iso;
}

// a cell has a vertex iff its corners are neither all inside nor all outside
DXV_HD bool iso_active(const float s[8])
{
    uint32_t n = 0;
    for (int k = 0; k < 8; ++k) n += iso_inside(s[k]) ? 1u : 0u;
    return n != 0u && n != 8u;
}
// the edges a cell owns run from its minimum corner along +x, +y, +z: bit a is set iff the one along axis a crosses
DXV_HD uint32_t iso_owned(const float s[8])
{
    const bool in0 = iso_inside(s[0]);
    return (in0 != iso_inside(s[1]) ? 1u : 0u) | (in0 != iso_inside(s[2]) ? 2u : 0u) | (in0 != iso_inside(s[4]) ? 4u : 0u);
}

// where an edge from a corner worth sa to the next one worth sb crosses, as a fraction of the edge
DXV_HD float iso_crossing(float sa, float sb) { return iso_finite(sa) && iso_finite(sb) ? sa / (sa - sb) : 0.5f; }

// the vertex of active cell (cx, cy, cz) in voxel index space (coordinate i = the centre of voxel i): the mean of the crossings of its
// twelve edges -- x edges, y edges, z edges, within an axis the other two offsets (0,0), (1,0), (0,1), (1,1) with the lower axis first --
// and the normalised sum of the edges' differences, which points towards growing values: out of the solid
DXV_HD IsoVertex iso_vertex(const float s[8], uint32_t cx, uint32_t cy, uint32_t cz)
{
    float sum[3] = {0.0f, 0.0f, 0.0f}, g[3] = {0.0f, 0.0f, 0.0f};
    uint32_t count = 0;
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (int axis = 0; axis < 3; ++axis) {
        const int lo = axis == 0 ? 1 : 0, hi = axis == 2 ? 1 : 2;
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
        for (int e = 0; e < 4; ++e) {
            const int a = ((e & 1) << lo) | ((e >> 1) << hi), b = a | (1 << axis);
            g[axis] = g[axis] + (s[b] - s[a]);
            if (iso_inside(s[a]) != iso_inside(s[b])) {
                const float t = iso_crossing(s[a], s[b]);
                sum[axis] = sum[axis] + t;
                sum[lo] = sum[lo] + (float)(e & 1);
                sum[hi] = sum[hi] + (float)(e >> 1);
                ++count;
            }
        }
    }
    const float n = (float)count;
    IsoVertex v;
    v.px = sum[0] / n + (float)((int32_t)cx - 1);
    v.py = sum[1] / n + (float)((int32_t)cy - 1);
    v.pz = sum[2] / n + (float)((int32_t)cz - 1);
    const float len2 = g[0] * g[0] + g[1] * g[1] + g[2] * g[2];
    v.nx = v.ny = v.nz = 0.0f;
    if (iso_finite(len2) && len2 > 0.0f) {
        const float len = sqrtf(len2);
        v.nx = g[0] / len; v.ny = g[1] / len; v.nz = g[2] / len;
    }
    return v;
}

// voxel index space -> object space: the voxel centres of the ray rules (y mirrored), times the scene's half extent, plus its centre
DXV_HD void iso_to_object(IsoVertex& v, uint32_t N, const float bound[4])
{
    const float n = (float)N;
    const float qx = (v.px + 0.5f) / n * 2.0f - 1.0f, qy = -((v.py + 0.5f) / n * 2.0f - 1.0f), qz = (v.pz + 0.5f) / n * 2.0f - 1.0f;
    v.px = qx * bound[3] + bound[0];
    v.py = qy * bound[3] + bound[1];
    v.pz = qz * bound[3] + bound[2];
    v.ny = -v.ny;
}

// the vertex number of cell (cx, cy, cz) from its word's bit mask and the vertices in front of the word
DXV_HD uint32_t iso_index(const uint64_t* masks, const IsoCounts* bases, uint32_t N, uint32_t cx, uint32_t cy, uint32_t cz)
{
    const size_t word = ((size_t)cz * (N + 1u) + cy) * iso_row_words(N) + (cx >> 6);
    return bases[word].vertices + iso_popc(masks[word] & ((1ull << (cx & 63u)) - 1ull));
}

// the quad of the crossing edge that cell c owns along `axis`: the four cells around the edge, c - u - w, c - w, c, c - u with u = axis + 1,
// w = axis + 2 (mod 3), in that cyclic order when the edge's first sample is inside, reversed otherwise; split (v0, v1, v2), (v0, v2, v3);
// in object space (y mirrored) every triangle (a, b, c) is written (c, b, a).  A crossing edge never lies in the outermost padding layer,
// so c - u and c - w exist.
DXV_HD void iso_quad(uint32_t out[6], const uint64_t* masks, const IsoCounts* bases, uint32_t N, uint32_t cx, uint32_t cy, uint32_t cz,
                     int axis, bool firstInside, bool object)
{
    const int u = (axis + 1) % 3, w = (axis + 2) % 3;
    const uint32_t c[3] = {cx, cy, cz};
    uint32_t q[4];
    for (int k = 0; k < 4; ++k) {
        uint32_t d[3] = {c[0], c[1], c[2]};
        if (k == 0 || k == 3) d[u] -= 1u;
        if (k == 0 || k == 1) d[w] -= 1u;
        q[k] = iso_index(masks, bases, N, d[0], d[1], d[2]);
    }
    const uint32_t v0 = firstInside ? q[0] : q[3], v1 = firstInside ? q[1] : q[2], v2 = firstInside ? q[2] : q[1], v3 = firstInside ? q[3] : q[0];
    if (!object) { out[0] = v0; out[1] = v1; out[2] = v2; out[3] = v0; out[4] = v2; out[5] = v3; }
    else { out[0] = v2; out[1] = v1; out[2] = v0; out[3] = v3; out[4] = v2; out[5] = v0; }
}

// ---- what isosurface.hip's launches work on: vb (24 bytes per vertex) and ib (three uint32 per triangle) are the caller's ----
struct IsoParams {
    const float* field;     // N^3 floats, element (iz * N + iy) * N + ix
    uint32_t N;
    float iso, P;           // the level, and one voxel in the field's unit: what a sample outside the grid is worth
    int object;             // 0: vertices in voxel index space, 1: in object space through `bound` (triangles turned round: y is mirrored)
    float bound[4];
    uint64_t* masks;        // iso_carve fills these four
    IsoCounts* bases;
    unsigned long long* sums;
    unsigned long long* totals;   // {vertices, quads} of the whole mesh
    IsoVertex* vb;
    uint32_t* ib;
};
// scratch of one extraction: one bit per lattice cell, two counts per 64 cells, the scan's block sums, the two totals -- 8-byte words one
// behind the other, not in lines of their own
inline void iso_carve(Carve& c, uint32_t N, IsoParams& p)
{
    const size_t words = iso_words(N);
    p.masks = reinterpret_cast<uint64_t*>(c.take_bytes(words * sizeof(uint64_t)));
    p.bases = reinterpret_cast<IsoCounts*>(c.take_bytes(words * sizeof(IsoCounts)));
    p.sums = reinterpret_cast<unsigned long long*>(c.take_bytes(2u * (size_t)scan_blocks(words) * sizeof(unsigned long long)));
    p.totals = reinterpret_cast<unsigned long long*>(c.take_bytes(2u * sizeof(unsigned long long)));
}
inline size_t iso_scratch_bytes(uint32_t N) { return carved_bytes<IsoParams>(iso_carve, N); }

} // namespace dxv
