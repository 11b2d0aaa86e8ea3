// dxv_distance.h -- the exact signed distance field of a grid (d2(p) = the smallest squared centre-to-centre distance from
// voxel p to a voxel of the OTHER kind, negative inside).  Integer geometry, separable: the nearest other voxel along x per row (bit
// scans over the row packed into 64-bit words), then a lower envelope of parabolas along y, then the same along z.  Everything here is
// __host__ __device__: distance.hip runs it on the GPU, tests/test_distance_rule.py compiles the same text for the CPU.
//
// Both signs in one run.  A voxel needs the nearest voxel of the other kind, so every pass would have to carry two fields (distance to
// the nearest solid, to the nearest empty voxel) -- but one of the two is always 0, the voxel's own kind, so ONE signed value per voxel
// carries both: magnitude = distance to the other kind, negative = solid.  And along a column only the voxel's own RUN of equal kind
// matters: a voxel of the same kind beyond the run's end lies behind a voxel of the other kind, which is nearer and costs nothing.  So
//     out(u) = min( (u - (a-1))^2 if a > 0,  ((b+1) - u)^2 if b < N-1,  min over j in [a, b] of (u - j)^2 + f(j) )
// for u in the run [a, b], f = the previous pass's magnitude.  The last term is Meijster's lower envelope (A. Meijster, J. Roerdink,
// W. Hesselink, "A general algorithm for computing distance transforms in linear time", 2000): a forward scan keeps the parabolas that
// are lowest somewhere on a stack, a backward scan reads the answers off it.
//
// No stack memory of its own: the stack of a run lives in the run's own slots of the OUTPUT column (32 bits per voxel).  Entry q
// (parabola s, lowest from t on) sits in slot a + q; s and t are both >= a + q, and the backward scan writes slot u only after every
// entry it still needs -- all of them in slots <= u, the one in slot u in registers -- so results overwrite the stack from the top.  The
// run's last parabola (b, f(b)) is never pushed but taken as a term of its own like the two neighbours of the run: the stack then has at
// most b - a entries and slot b is free for the run's marker (a, entries), which the backward scan reads when it enters the run from
// above.  An entry does not hold f(s) (11 + 11 + 23 bits do not fit): it is read again from the input column when the entry becomes the
// top, so the input of a pass is never its output.
#pragma once
#include <math.h>
#include "dxv_types.h"
#include "dxv_scratch.h"

namespace dxv {

constexpr int32_t kDistNone = 0x7fffffff;     // magnitude where no voxel of the other kind exists (the int32 format's own sentinel)
constexpr int32_t kDistRowNone = 0x7fff;      // ... in the 16-bit values of the x pass

// scratch of the three passes: the x pass's 16-bit values in whole lines, the y pass's squares as they are (the one block of the operators
// that does not end on a line: what embeds these passes puts them last)
struct DistScratch { int16_t* rows; int32_t* squares; };
inline void distance_carve(Carve& c, uint32_t N, DistScratch& l)
{
    const size_t voxels = (size_t)N * N * N;
    l.rows = c.take<int16_t>(voxels);
    l.squares = reinterpret_cast<int32_t*>(c.take_bytes(voxels * sizeof(int32_t)));
}
inline size_t distance_scratch_bytes(uint32_t N) { return carved_bytes<DistScratch>(distance_carve, N); }

// ---- x: the nearest voxel of the other kind in the row.  bits: the row's voxels, bit x % 64 of word x / 64 set = solid ----
DXV_HD uint64_t dist_row_other(const uint64_t* bits, uint32_t N, uint32_t w, bool solid)
{
    const uint32_t rest = N - 64u * w;                                   // voxels from this word on: the row's last word may be partial
    const uint64_t valid = rest >= 64u ? ~0ull : (1ull << rest) - 1ull;
    return (solid ? ~bits[w] : bits[w]) & valid;
}
// signed 16-bit value of voxel x: +distance for an empty voxel, -distance for a solid one, magnitude kDistRowNone when the row is all one kind
DXV_HD int32_t dist_row_value(const uint64_t* bits, uint32_t N, uint32_t x, bool solid)
{
    const uint32_t W = (N + 63u) / 64u, c = x >> 6, l = x & 63u;
    uint32_t best = (uint32_t)kDistRowNone;
    uint64_t m = dist_row_other(bits, N, c, solid) >> l;                // (the voxel's own bit is not of the other kind)
    if (m) best = (uint32_t)__builtin_ctzll(m);
    else
        for (uint32_t w = c + 1u; w < W; ++w) {
            m = dist_row_other(bits, N, w, solid);
            if (m) { best = w * 64u + (uint32_t)__builtin_ctzll(m) - x; break; }
        }
    m = dist_row_other(bits, N, c, solid) << (63u - l);
    uint32_t left = (uint32_t)kDistRowNone;
    if (m) left = (uint32_t)__builtin_clzll(m);
    else
        for (uint32_t w = c; w-- > 0u;) {
            m = dist_row_other(bits, N, w, solid);
            if (m) { left = x - (w * 64u + 63u - (uint32_t)__builtin_clzll(m)); break; }
        }
    if (left < best) best = left;
    return solid ? -(int32_t)best : (int32_t)best;
}

// ---- y, z: what a column reads -- the x pass's signed distances (squared here), or the y pass's signed squares as they are ----
DXV_HD int32_t dist_square_of(int16_t g)
{
    const int32_t m = g < 0 ? -(int32_t)g : (int32_t)g;
    const int32_t sq = m == kDistRowNone ? kDistNone : m * m;
    return g < 0 ? -sq : sq;
}
DXV_HD int32_t dist_square_of(int32_t h) { return h; }
DXV_HD int32_t dist_float_bits(float f)
{
    int32_t i;
    __builtin_memcpy(&i, &f, 4);
    return i;
}

// One column of N values `stride` elements apart: in -> out (never the same memory).  kFloat = false: signed squares, the input of the
// next pass and DXV_DIST_SQ_I32 itself; true: DXV_DIST_F32, the bits of s * sqrtf((float)d2), s * INFINITY where there is none.
// Magnitudes stay below 3 * 2047^2 < 2^24 and every intermediate below 2^26: int32 throughout.
template <class TIn, bool kFloat> struct DistColumn {
    const TIn* in;
    int32_t* out;
    size_t stride;
    int32_t N;
    int32_t a = 0, q = -1;                      // the run's first voxel; top of its stack (-1: empty)
    int32_t ts = 0, tt = 0, tf = 0;             // the top entry: parabola ts of height tf is the lowest one from tt on

    DXV_HD static int32_t mag(int32_t v) { return v < 0 ? -v : v; }
    DXV_HD int32_t value(int32_t u) const { return dist_square_of(in[(size_t)u * stride]); }
    DXV_HD void load_top()
    {
        const uint32_t e = (uint32_t)out[(size_t)(a + q) * stride];
        ts = (int32_t)(e & 0xffffu); tt = (int32_t)(e >> 16);
        if (ts > N - 1) ts = N - 1;             // (what this scan wrote itself is in range: no read ever leaves the column, whatever the memory holds)
        tf = mag(value(ts));
    }
    DXV_HD void pop() { if (--q >= 0) load_top(); }
    // parabola (u, f), f finite, u beyond every parabola of the stack
    DXV_HD void push(int32_t u, int32_t f)
    {
        while (q >= 0 && (tt - ts) * (tt - ts) + tf > (tt - u) * (tt - u) + f) pop();
        // the first voxel where u is lower than the top: 1 + the largest x with (x - ts)^2 + tf <= (x - u)^2 + f (>= tt: the numerator is not negative)
        const int32_t w = q < 0 ? a : 1 + (u * u - ts * ts + f - tf) / (2 * (u - ts));
        if (w < N) {
            ++q; ts = u; tt = w; tf = f;
            out[(size_t)(a + q) * stride] = (int32_t)((uint32_t)u | ((uint32_t)w << 16));
        }
    }
    // the run [a, b] is complete: entries that start beyond it go, its marker goes into slot b
    DXV_HD void finish(int32_t b)
    {
        while (q >= 0 && tt > b) pop();
        out[(size_t)b * stride] = (int32_t)((uint32_t)a | ((uint32_t)(q + 1) << 16));
    }
    DXV_HD void run()
    {
        int32_t pv = value(0);
        for (int32_t u = 1; u < N; ++u) {
            const int32_t v = value(u);
            if ((v < 0) != (pv < 0)) { finish(u - 1); a = u; q = -1; }
            else if (mag(pv) != kDistNone) push(u - 1, mag(pv));
            pv = v;
        }
        finish(N - 1);
        int32_t b = N - 1, fb = 0, nv = 0;
        for (int32_t u = N - 1; u >= 0; --u) {
            const int32_t v = value(u);
            const bool solid = v < 0;
            if (u == N - 1 || (nv < 0) != solid) {                      // a run entered from above: its marker, its top entry
                b = u; fb = mag(v);
                const uint32_t e = (uint32_t)out[(size_t)u * stride];
                a = (int32_t)(e & 0xffffu); q = (int32_t)(e >> 16);
                if (a > u) a = u;
                if (q > u - a) q = u - a;
                --q;
                if (q >= 0) load_top();
            }
            int32_t best = kDistNone;
            if (q >= 0) best = (u - ts) * (u - ts) + tf;
            if (fb != kDistNone && (b - u) * (b - u) + fb < best) best = (b - u) * (b - u) + fb;
            if (a > 0 && (u - a + 1) * (u - a + 1) < best) best = (u - a + 1) * (u - a + 1);
            if (b < N - 1 && (b + 1 - u) * (b + 1 - u) < best) best = (b + 1 - u) * (b + 1 - u);
            if (kFloat) {
                const float d = best == kDistNone ? __builtin_inff() : sqrtf((float)best);
                out[(size_t)u * stride] = dist_float_bits(solid ? -d : d);
            }
            else out[(size_t)u * stride] = solid ? -best : best;
            if (q >= 0 && u == tt) pop();
            nv = v;
        }
    }
};

} // namespace dxv
