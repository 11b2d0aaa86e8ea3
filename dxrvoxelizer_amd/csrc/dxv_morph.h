// dxv_morph.h -- growing and shrinking the solid of a grid by the exact Euclidean ball (B = { v in Z^3 : |v|^2 <= r2 };
// DILATE(p) iff a solid q of the grid has |p - q|^2 <= r2, ERODE(p) iff p is solid and no empty q of the grid has; OPEN = DILATE(ERODE),
// CLOSE = ERODE(DILATE); voxels outside the grid do not exist) on BITS, in the fill's mask layout (dxv_fill.h: rows of fill_row_words(N)
// 64-bit words, the bits behind a row's end 0).  ONE primitive, the dilation of a member mask; ERODE is the dilation of the complement taken
// inside the grid, complemented again inside the grid -- padding that looked empty would erode the grid's border.
//
// The ball is a stack of discs and a disc a stack of segments: p is in the dilation iff for some (dy, dz) with dy^2 + dz^2 <= r2 the row
// (y + dy, z + dz) has a member within k(dy, dz) = floor(sqrt(r2 - dy^2 - dz^2)) of p along x.  So
//     plane_k  = the mask spread by k along x, k = 0 .. R = floor(sqrt(r2))     (plane_k = plane_{k-1} | the row shifted by k either way)
//     out(row) = OR over (dy, dz) of plane_{k(dy, dz)}(row + (dy, dz))          (rows outside the grid contribute nothing)
// and every operation is on whole 64-bit words: the second line costs one load and one OR per offset and 64 voxels, about pi r2 of them.
// Everything here is __host__ __device__: morph.hip runs it on the GPU, tests/test_morph_rule.py compiles the same text for the CPU.
#pragma once
#include <math.h>
#include <stddef.h>
#include "dxv_types.h"
#include "dxv_solid.h"
#include "dxv_fill.h"
#include "dxv_distance.h"

namespace dxv {

enum { MORPH_DILATE = 0, MORPH_ERODE = 1, MORPH_OPEN = 2, MORPH_CLOSE = 3 };
constexpr uint32_t kMorphMaxRadiusSq = 4096;      // the ball reaches at most one mask word along x (R <= 64)
constexpr uint32_t kMorphMaxN = 2048;             // the library's largest grid: mask words and groups of eight voxels fit 32 bits

// Two forms, the same bytes.  MORPH_FORM_PLANES: the word-parallel form above, pi r2 loads per 64 voxels -- a fraction of a distance field at
// small radii, one field at r2 = 784 and 4.2 of them at 4096 (profiles/NOTES.md, "Morphology").  MORPH_FORM_FIELD: per
// half the exact field of the grid (distance.hip, whose cost does not depend on the radius) and its threshold, by the identity
//     DILATE(p) == solid(p) || d(p) <= r2          ERODE(p) == solid(p) && -d(p) > r2          d = DXV_DIST_SQ_I32
// 1.2 - 1.35 fields per half at every radius.  The two forms cost the same at r2 = 1024, which is where the library changes over.
enum { MORPH_FORM_AUTO = 0, MORPH_FORM_PLANES = 1, MORPH_FORM_FIELD = 2 };
constexpr uint32_t kMorphPlanesMaxRadiusSq = 1024; // the largest radius the planes take when nobody says otherwise (option morphform)
DXV_HD int morph_form(uint32_t r2, int asked) { return asked != MORPH_FORM_AUTO ? asked : r2 > kMorphPlanesMaxRadiusSq ? MORPH_FORM_FIELD : MORPH_FORM_PLANES; }
// the field form's halves: is half `half` of op an erosion
DXV_HD bool morph_half_erodes(int op, uint32_t half) { return op == MORPH_ERODE || (op == MORPH_OPEN && half == 0u) || (op == MORPH_CLOSE && half == 1u); }
// ... and one voxel of its threshold: the byte it becomes (0 / 1) from its signed squared distance (negative: solid)
DXV_HD uint32_t morph_threshold(int32_t d, uint32_t r2, bool erode)
{
    const bool solid = d < 0;
    const uint32_t mag = (uint32_t)(solid ? -d : d);                    // (the sentinel 0x7fffffff is beyond every radius)
    return erode ? (solid && mag > r2 ? 1u : 0u) : (solid || mag <= r2 ? 1u : 0u);
}

// floor(sqrt(v)), v <= kMorphMaxRadiusSq: the correctly rounded float root of an integer below 2^24, put right if it is one off
DXV_HD uint32_t morph_isqrt(uint32_t v)
{
    uint32_t r = (uint32_t)sqrtf((float)v);
    if (r * r > v) --r;
    if ((r + 1u) * (r + 1u) <= v) ++r;
    return r;
}
// the voxels of word w of a row that exist
DXV_HD uint64_t morph_valid(uint32_t N, uint32_t w)
{
    const uint32_t rest = N - 64u * w;
    return rest >= 64u ? ~0ull : (1ull << rest) - 1ull;
}
// the halves of an operation: what the pack takes as members, and whether each dilation's result is complemented (inside the grid).
//   DILATE: D(S)            ERODE: ~D(~S)            OPEN: D(~D(~S))            CLOSE: ~D(~D(S)) -- its first half leaves ~D(S), the
// members of its second
DXV_HD bool morph_packs_complement(int op) { return op == MORPH_ERODE || op == MORPH_OPEN; }
DXV_HD uint32_t morph_halves(int op) { return op == MORPH_OPEN || op == MORPH_CLOSE ? 2u : 1u; }
DXV_HD bool morph_half_complements(int op, uint32_t half) { return op == MORPH_ERODE || op == MORPH_CLOSE || (op == MORPH_OPEN && half == 0u); }

// ---- pack: eight voxels -> one byte of the member mask (the solid voxels, or the empty ones that exist).  j: the byte's place in its row ----
DXV_HD uint32_t morph_member_byte(const uint8_t* row, uint32_t N, uint32_t j, bool complement)
{
    const uint32_t left = N - 8u * j, valid = left >= 8u ? 0xffu : (1u << left) - 1u;
    const uint32_t s = solid_bits(row + 8u * j, left);
    return (complement ? ~s : s) & valid;
}
// ... from eight bytes loaded as one word (N % 8 == 0)
DXV_HD uint32_t morph_member_byte(uint64_t eight, bool complement) { return (complement ? ~solid_bits(eight) : solid_bits(eight)) & 0xffu; }
// one of the eight is neither 0 nor 1: the write-back has to store these eight even where no voxel changes kind
DXV_HD bool morph_loose(uint64_t eight) { return (eight & ~0x0101010101010101ull) != 0ull; }
DXV_HD bool morph_loose(const uint8_t* row, uint32_t N, uint32_t j)
{
    bool loose = false;
    for (uint32_t k = 0; k < 8u && 8u * j + k < N; ++k) loose |= row[8u * j + k] > 1u;
    return loose;
}

// ---- x: the members of a row at distance exactly k (1 .. 64) from the voxels of word m; prev, next: the words beside it (0 at the row's ends) ----
DXV_HD uint64_t morph_shifted(uint64_t prev, uint64_t m, uint64_t next, uint32_t k)
{
    if (k >= 64u) return prev | next;
    return (m << k) | (prev >> (64u - k)) | (m >> k) | (next << (64u - k));
}

// ---- y, z: one word of the dilation.  m0: plane 0, the mask itself; planes: plane k at planes + (k - 1) * words, k = 1 .. R; t: the word
// (z * N + y) * W + w.  Every load stays in the planes: a row outside the grid is skipped, bits that were spread behind a row's end are for
// the caller to clear (morph_valid). ----
DXV_HD uint64_t morph_ball_word(const uint64_t* m0, const uint64_t* planes, size_t words, uint32_t N, uint32_t W, uint32_t r2, uint32_t y, uint32_t z, size_t t)
{
    const int32_t R = (int32_t)morph_isqrt(r2);
    uint64_t acc = 0;
    for (int32_t dz = -R; dz <= R; ++dz) {
        if ((uint32_t)((int32_t)z + dz) >= N) continue;
        const uint32_t s = r2 - (uint32_t)(dz * dz);                    // what is left for dy^2 + k^2
        const size_t at = (size_t)((ptrdiff_t)t + (ptrdiff_t)dz * (ptrdiff_t)N * (ptrdiff_t)W);
        uint32_t k = morph_isqrt(s);
        for (uint32_t dy = 0; dy * dy <= s; ++dy) {
            while (k * k > s - dy * dy) --k;                            // k = floor(sqrt(s - dy^2)): falls as dy grows
            const uint64_t* plane = k ? planes + (size_t)(k - 1u) * words : m0;
            if (y + dy < N) acc |= plane[at + (size_t)dy * W];
            if (dy && y >= dy) acc |= plane[at - (size_t)dy * W];
        }
    }
    return acc;
}

// ---- write-back: one byte of the masks -> eight result bytes of 0 / 1 (fill_spread_byte), and what it counts ----
DXV_HD uint32_t morph_popc8(uint32_t b) { return solid_popc((uint64_t)(b & 0xffu)); }

// ---- scratch of one call: {voxels set, voxels cleared} in a line of their own, then
//   planes: the packed mask, one result mask per half, the "neither 0 nor 1" bits, the R planes (a mask each)
//   field:  the field (4 B per voxel) and the scratch of its passes (distance_scratch_bytes, 6 B per voxel) ----
struct MorphScratch {
    unsigned long long* counters;
    uint64_t *packed, *half[2], *loose, *planes;
    int32_t* field;
    uint8_t* passes;
};
inline void morph_carve(Carve& c, uint32_t N, int op, uint32_t r2, int form, MorphScratch& l)
{
    l.counters = reinterpret_cast<unsigned long long*>(c.take_bytes(256u));
    if (form == MORPH_FORM_FIELD) {
        l.field = c.take<int32_t>((size_t)N * N * N);
        l.passes = c.take_bytes(distance_scratch_bytes(N));
        return;
    }
    l.packed = c.take<uint64_t>(fill_mask_words(N));
    for (uint32_t half = 0; half < morph_halves(op); ++half) l.half[half] = c.take<uint64_t>(fill_mask_words(N));
    l.loose = c.take<uint64_t>(fill_loose_words(N));
    l.planes = reinterpret_cast<uint64_t*>(c.take_bytes((size_t)morph_isqrt(r2) * fill_mask_bytes(N)));
}
inline size_t morph_scratch_bytes(uint32_t N, int op, uint32_t r2, int form) { return carved_bytes<MorphScratch>(morph_carve, N, op, r2, form); }

} // namespace dxv
