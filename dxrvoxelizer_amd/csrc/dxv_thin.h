// dxv_thin.h -- topology-preserving thinning of a grid's solid (voxels outside the grid are EMPTY; p is simple iff
// T26(p) == 1 && T6(p) == 1; one iteration = the border B as it is at its start, then the eight subfields sub(p) = (x & 1) | (y & 1) << 1 |
// (z & 1) << 2 in the order 0 .. 7, each removing at once its voxels that are in B, still solid, simple in the current solid set and not kept by
// the kind) on BITS, in the fill's mask layout (dxv_fill.h: rows of fill_row_words(N) 64-bit words, the bits behind a row's end 0).
//
// THE CONFIGURATION of a voxel p is a 27-bit word, one bit per voxel of the 3 x 3 x 3 block around p:
//     bit (dz + 1) * 9 + (dy + 1) * 3 + (dx + 1) is set iff p + (dx, dy, dz) is solid        dx, dy, dz in {-1, 0, 1}
// so x runs fastest, as in the grid, and bit 13 -- p itself -- is always 0: 26 bits carry something.  Everything below is switch-free bit
// arithmetic on such words: a set of the block's voxels grows by one step along an axis through two shifts and two masks, so no table is
// indexed by a lane's value and nothing goes to scratch memory.  A flood inside the block gains at least one of 26 voxels per step.
// Everything here is __host__ __device__: thin.hip runs it on the GPU, tests/test_thin_rule.py compiles the same text for the CPU.
#pragma once
#include <stddef.h>
#include "dxv_types.h"
#include "dxv_solid.h"
#include "dxv_fill.h"

namespace dxv {

enum { THIN_CURVE = 0, THIN_KERNEL = 1 };
constexpr uint32_t kThinMaxN = 2048;              // the library's largest grid: mask words fit 32 bits
constexpr uint32_t kThinMaxRounds = 64;           // iterations of one batch at the most (option thinrounds); words of the batch's control block
constexpr uint32_t kThinRoundsDefault = 16;       // ... by default (profiles/NOTES.md, "Thinning": the bunny at 256^3 gains nothing beyond it)

// ---- the block's masks ----
constexpr uint32_t thin_bit(int dx, int dy, int dz) { return 1u << ((dz + 1) * 9 + (dy + 1) * 3 + (dx + 1)); }
constexpr uint32_t thin_mask(int minSum, int maxSum, int axis = -1, int at = 0)    // the voxels with minSum <= |dx| + |dy| + |dz| <= maxSum (and coordinate `axis` == at)
{
    uint32_t m = 0;
    for (int dz = -1; dz <= 1; ++dz)
        for (int dy = -1; dy <= 1; ++dy)
            for (int dx = -1; dx <= 1; ++dx) {
                const int sum = (dx < 0 ? -dx : dx) + (dy < 0 ? -dy : dy) + (dz < 0 ? -dz : dz);
                const int c = axis == 0 ? dx : axis == 1 ? dy : dz;
                if (sum >= minSum && sum <= maxSum && (axis < 0 || c == at)) m |= thin_bit(dx, dy, dz);
            }
    return m;
}
constexpr uint32_t kThinN26 = thin_mask(1, 3);    // everything but p
constexpr uint32_t kThinN18 = thin_mask(1, 2);    // ... that shares a face or an edge with p
constexpr uint32_t kThinN6 = thin_mask(1, 1);     // ... a face
constexpr uint32_t kThinXLo = thin_mask(0, 3, 0, -1), kThinXHi = thin_mask(0, 3, 0, 1);
constexpr uint32_t kThinYLo = thin_mask(0, 3, 1, -1), kThinYHi = thin_mask(0, 3, 1, 1);
constexpr uint32_t kThinAll = thin_mask(0, 3);
static_assert(kThinAll == 0x7ffffffu && kThinN26 == (kThinAll & ~(1u << 13)), "27 bits, p in the middle");
static_assert(kThinXLo == 0x1249249u && kThinYLo == 0x1c0e07u && kThinN6 == ((1u << 4) | (1u << 10) | (1u << 12) | (1u << 14) | (1u << 16) | (1u << 22)), "x fastest");

// a set of the block's voxels and what is one step from it along x, y, z (a shift moves a whole row or slice; the masks keep a row's and a
// slice's last voxel from wrapping into the next)
DXV_HD uint32_t thin_step_x(uint32_t m) { return ((m & ~kThinXHi) << 1) | ((m & ~kThinXLo) >> 1); }
DXV_HD uint32_t thin_step_y(uint32_t m) { return ((m & ~kThinYHi) << 3) | ((m & ~kThinYLo) >> 3); }
DXV_HD uint32_t thin_step_z(uint32_t m) { return ((m << 9) | (m >> 9)) & kThinAll; }
// ... with everything 6-adjacent to it, and everything 26-adjacent (the three axes one after the other: the whole 3 x 3 x 3 box round every voxel)
DXV_HD uint32_t thin_grow6(uint32_t m) { return m | thin_step_x(m) | thin_step_y(m) | thin_step_z(m); }
DXV_HD uint32_t thin_grow26(uint32_t m)
{
    m |= thin_step_x(m);
    m |= thin_step_y(m);
    return m | thin_step_z(m);
}
DXV_HD uint32_t thin_lowest(uint32_t m) { return m & (0u - m); }
DXV_HD uint32_t thin_popc(uint32_t m) { return solid_popc((uint64_t)m); }
// the members of `within` that paths through `within` join to `seed`
template <bool k26> DXV_HD uint32_t thin_flood(uint32_t seed, uint32_t within)
{
    uint32_t r = seed & within;
    for (uint32_t step = 0; step < 26u; ++step) {
        const uint32_t n = (k26 ? thin_grow26(r) : thin_grow6(r)) & within;
        if (n == r) break;
        r = n;
    }
    return r;
}

// ---- the two counts ----
// T26: the 26-connected components of the solid voxels of N26*(p)
DXV_HD uint32_t thin_T26(uint32_t cfg)
{
    uint32_t left = cfg & kThinN26, count = 0;
    while (left) {
        left &= ~thin_flood<true>(thin_lowest(left), left);
        ++count;
    }
    return count;
}
// T6: the 6-connected components of the empty voxels of N18*(p) that contain a voxel of N6*(p)
DXV_HD uint32_t thin_T6(uint32_t cfg)
{
    const uint32_t empty = ~cfg & kThinN18;
    uint32_t left = empty & kThinN6, count = 0;
    while (left) {
        left &= ~thin_flood<false>(thin_lowest(left), empty);
        ++count;
    }
    return count;
}
// simple: both counts are 1 -- one flood each: the component of the lowest voxel is all there is
DXV_HD bool thin_simple(uint32_t cfg)
{
    const uint32_t solid = cfg & kThinN26, empty = ~cfg & kThinN18, faces = empty & kThinN6;
    if (!solid || !faces) return false;                                 // T26 == 0: p alone; T6 == 0: no face neighbour is empty, p is not in B
    if (thin_flood<true>(thin_lowest(solid), solid) != solid) return false;
    return (faces & ~thin_flood<false>(thin_lowest(faces), empty)) == 0u;
}
// what the kind keeps whatever its counts: CURVE the end of a curve, exactly one solid voxel in N26*(p); KERNEL nothing
DXV_HD bool thin_keeps(int kind, uint32_t cfg) { return kind == THIN_CURVE && thin_popc(cfg & kThinN26) == 1u; }
DXV_HD bool thin_removes(int kind, uint32_t cfg) { return !thin_keeps(kind, cfg) && thin_simple(cfg); }

// ---- the border: the voxels of word s with an empty face neighbour.  prev, next: the words beside it in its row (0 at the row's ends, and a
// row's bits behind its end are 0: the row's last voxel is border); ym, yp, zm, zp: the same word of the rows at y -+ 1, z -+ 1 (0 outside the grid) ----
DXV_HD uint64_t thin_border_word(uint64_t s, uint64_t prev, uint64_t next, uint64_t ym, uint64_t yp, uint64_t zm, uint64_t zp)
{
    const uint64_t xm = (s << 1) | (prev >> 63), xp = (s >> 1) | (next << 63);
    return s & ~(xm & xp & ym & yp & zm & zp);
}

// ---- the configuration: one row of the nine as a window of 66 bits, voxel x of the word at window bit x + 1 ----
struct ThinRow {
    uint64_t lo;            // window bits 0 .. 63: voxel -1 (bit 63 of the word before) and voxels 0 .. 62
    uint32_t hi;            // window bits 64, 65: voxel 63 and voxel 64 (bit 0 of the word behind)
};
DXV_HD ThinRow thin_row(uint64_t prev, uint64_t cur, uint64_t next) { return {(cur << 1) | (prev >> 63), (uint32_t)(cur >> 63) | ((uint32_t)(next & 1ull) << 1)}; }
// the three voxels b - 1, b, b + 1 of the row, b = 0 .. 63: crosses into the word before at b = 0 and into the word behind at b = 63
DXV_HD uint32_t thin_three(const ThinRow& r, uint32_t b)
{
    const uint64_t top = b >= 62u ? (uint64_t)r.hi << (64u - b) : 0ull;
    return (uint32_t)((r.lo >> b) | top) & 7u;
}
// rows[(dz + 1) * 3 + (dy + 1)]: the nine rows round voxel b of the middle one
DXV_HD uint32_t thin_config(const ThinRow* rows, uint32_t b)
{
    uint32_t cfg = 0;
#pragma unroll
    for (uint32_t k = 0; k < 9u; ++k) cfg |= thin_three(rows[k], b) << (3u * k);
    return cfg & kThinN26;
}
// the bits of a word that belong to the subfields with x & 1 == odd
DXV_HD uint64_t thin_x_parity(uint32_t odd) { return odd ? 0xaaaaaaaaaaaaaaaaull : 0x5555555555555555ull; }

// ---- one word of one sub-iteration: the candidates among its voxels, decided one after the other from the nine rows.  Returns the word as it
// is afterwards; removing a candidate changes no other candidate's configuration (two voxels of one subfield are never 26-adjacent), so the
// rows need no update in between. ----
DXV_HD uint64_t thin_word(uint64_t s, uint64_t border, const ThinRow* rows, uint32_t xOdd, int kind)
{
    uint64_t cand = s & border & thin_x_parity(xOdd);
    while (cand) {
        const uint64_t low = cand & (0ull - cand);
        cand ^= low;
        const uint32_t b = solid_popc(low - 1ull);
        if (thin_removes(kind, thin_config(rows, b))) s ^= low;
    }
    return s;
}

// ---- batches: how many iterations the next batch runs.  left: what max_iterations still allows (0: no bound) ----
DXV_HD uint32_t thin_batch(uint32_t rounds, uint32_t left)
{
    if (rounds < 1u) rounds = 1u;
    if (rounds > kThinMaxRounds) rounds = kThinMaxRounds;
    return left && left < rounds ? left : rounds;
}

// ---- scratch of thin.hip ----
// the batch's control block -- word k != 0: iteration k removed something; the batch has reached the fixed point exactly when one of its words is
// 0 -- and the voxels removed since the first batch
struct ThinControl {
    uint32_t live[64];                // (kThinMaxRounds)
    unsigned long long removed;
    unsigned long long written[2];    // the write-back's own counters: nobody reads them
};
constexpr size_t kThinControlBytes = 512;
static_assert(sizeof(ThinControl) <= kThinControlBytes && sizeof(ThinControl::live) == sizeof(uint32_t) * kThinMaxRounds, "the control block has a word per iteration of a batch");
// the control block, S, S as it was, B, the loose bits: 3 1/8 bits per voxel
struct ThinScratch { ThinControl* ctl; uint64_t *S, *was, *B, *loose; };
inline void thin_carve(Carve& c, uint32_t N, ThinScratch& l)
{
    l.ctl = reinterpret_cast<ThinControl*>(c.take_bytes(kThinControlBytes));
    l.S = c.take<uint64_t>(fill_mask_words(N));
    l.was = c.take<uint64_t>(fill_mask_words(N));
    l.B = c.take<uint64_t>(fill_mask_words(N));
    l.loose = c.take<uint64_t>(fill_loose_words(N));
}
inline size_t thin_scratch_bytes(uint32_t N) { return carved_bytes<ThinScratch>(thin_carve, N); }

} // namespace dxv
