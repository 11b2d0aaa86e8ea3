// dxv_fill.h -- the exterior flood fill of a grid (outside = the free voxels a 6-connected path of free voxels joins to a
// free voxel on the grid's border; everything else is solid) on BITS: a free mask F and a reached mask R, one bit per voxel, rows of
// fill_row_words(N) 64-bit words (bit x % 64 of word x / 64; the bits behind the row's end are 0 in both), word (iz * N + iy) * W + w.
// R starts as the free voxels of the border and only grows, always inside F.  One ROUND is three passes, each of them forward and
// backward along its axis: the rows along x (carries from word to word), then one lane per 64-bit word column along y, then along z.
// A round that changes no word has found the fixed point, and the fixed point is the rule's smallest set: R grows only through face
// neighbours in F, so it never leaves it, and a fixed point of all six directions that holds the seeds contains it.
// Everything here is __host__ __device__: fill.hip runs it on the GPU, tests/test_fill_rule.py compiles the same text for the CPU.
#pragma once
#include <stddef.h>
#include "dxv_types.h"
#include "dxv_solid.h"
#include "dxv_scratch.h"

namespace dxv {

constexpr uint32_t kFillMaxRounds = 64;           // rounds of one batch at the most (option fillrounds); words of the batch's control block
constexpr uint32_t kFillRoundsDefault = 4;        // ... by default (profiles/NOTES.md, "Flood fill": the meshes measured take 2 - 3)
constexpr uint32_t kFillBlock = 8;                // steps of a column pass whose loads are issued together, in front of the chain through them

DXV_HD uint32_t fill_row_words(uint32_t N) { return (N + 63u) / 64u; }
DXV_HD size_t fill_mask_words(uint32_t N) { return (size_t)N * N * fill_row_words(N); }
// such a mask in whole lines of device memory, and beside it one bit per eight voxels of it (morph.hip's pack: "a byte here is neither 0 nor 1")
inline size_t fill_loose_words(uint32_t N) { return (fill_mask_words(N) * 8u + 63u) / 64u; }
inline size_t fill_mask_bytes(uint32_t N) { return align256(fill_mask_words(N) * sizeof(uint64_t)); }
inline size_t fill_loose_bytes(uint32_t N) { return align256(fill_loose_words(N) * sizeof(uint64_t)); }

// scratch of the fill: the free mask, the reached mask, the batch's control block (a word per round)
struct FillScratch { uint64_t *freeMask, *reached; uint32_t* ctl; };
inline void fill_carve(Carve& c, uint32_t N, FillScratch& l)
{
    l.freeMask = c.take<uint64_t>(fill_mask_words(N));
    l.reached = c.take<uint64_t>(fill_mask_words(N));
    l.ctl = reinterpret_cast<uint32_t*>(c.take_bytes(sizeof(uint32_t) * kFillMaxRounds));
}
inline size_t fill_scratch_bytes(uint32_t N) { return carved_bytes<FillScratch>(fill_carve, N); }

DXV_HD uint64_t fill_reverse(uint64_t v)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return __brevll(v);
#else
    v = __builtin_bswap64(v);
    v = ((v >> 4) & 0x0f0f0f0f0f0f0f0full) | ((v & 0x0f0f0f0f0f0f0f0full) << 4);
    v = ((v >> 2) & 0x3333333333333333ull) | ((v & 0x3333333333333333ull) << 2);
    return ((v >> 1) & 0x5555555555555555ull) | ((v & 0x5555555555555555ull) << 1);
#endif
}
// the bits of f that a run of set bits of f joins to a bit of r from BELOW (r itself included): adding r to f sends a carry from a run's
// lowest bit of r to the run's end, which flips exactly the bits it passes; the run's other bits of r come back with the OR
DXV_HD uint64_t fill_up(uint64_t r, uint64_t f)
{
    r &= f;
    return f & (((f + r) ^ f) | r);
}
DXV_HD uint64_t fill_down(uint64_t r, uint64_t f) { return fill_reverse(fill_up(fill_reverse(r), fill_reverse(f))); }
// every run of f that holds a bit of r, whole
DXV_HD uint64_t fill_word(uint64_t r, uint64_t f) { return fill_up(r, f) | fill_down(r, f); }

// ---- pack: eight voxels -> one byte of F and one of R's seed.  j: the byte's place in its row (voxels 8j .. 8j+7) ----
DXV_HD uint32_t fill_free_byte(const uint8_t* row, uint32_t N, uint32_t j)
{
    uint32_t b = 0;
    for (uint32_t k = 0; k < 8u; ++k) {
        const uint32_t x = 8u * j + k;
        if (x < N && !solid(row[x])) b |= 1u << k;
    }
    return b;
}
// ... from eight bytes loaded as one word (N % 8 == 0: every row starts on an 8-byte boundary of the grid): bit k = byte k is zero,
// the complement of the library's solid rule (dxv_solid.h)
DXV_HD uint32_t fill_free_byte(uint64_t eight) { return ~solid_bits(eight) & 0xffu; }
// the free voxels of the grid's border among these eight
DXV_HD uint32_t fill_seed_byte(uint32_t free8, uint32_t N, uint32_t j, uint32_t iy, uint32_t iz)
{
    if (iy == 0 || iz == 0 || iy == N - 1u || iz == N - 1u) return free8;
    uint32_t m = j == 0 ? 1u : 0u;
    if ((N - 1u) >> 3 == j) m |= 1u << ((N - 1u) & 7u);
    return free8 & m;
}

// ---- x: one row of W words, forward with the carry out of bit 63, then backward with the carry out of bit 0 ----
DXV_HD bool fill_row(const uint64_t* f, uint64_t* r, uint32_t W)
{
    bool changed = false;
    uint64_t carry = 0;
    for (uint32_t w = 0; w < W; ++w) {
        const uint64_t old = r[w], now = fill_word(old | carry, f[w]);
        if (now != old) { r[w] = now; changed = true; }
        carry = now >> 63;
    }
    carry = 0;
    for (uint32_t w = W; w-- > 0u;) {
        const uint64_t old = r[w], now = fill_word(old | carry, f[w]);
        if (now != old) { r[w] = now; changed = true; }
        carry = (now & 1ull) << 63;
    }
    return changed;
}

// ---- y, z: one column of N words `stride` words apart, forward then backward: a word takes what the word before it reached, through
// its own free bits, and spreads it along x inside itself.  The addresses do not depend on the values: the loads of kFillBlock steps are
// issued together and the chain runs through registers. ----
struct FillColumn {
    const uint64_t* f;
    uint64_t* r;
    size_t stride;
    uint32_t N;
    bool changed = false;

    DXV_HD uint64_t step(size_t u, uint64_t fw, uint64_t old, uint64_t prev)
    {
        const uint64_t now = fill_word(old | prev, fw);
        if (now != old) { r[u * stride] = now; changed = true; }
        return now;
    }
    template <bool kForward> DXV_HD void pass()
    {
        uint64_t prev = 0;
        uint32_t done = 0;
        for (; done + kFillBlock <= N; done += kFillBlock) {
            uint64_t fw[kFillBlock], rw[kFillBlock];
#pragma unroll
            for (uint32_t k = 0; k < kFillBlock; ++k) {
                const size_t u = kForward ? done + k : N - 1u - done - k;
                fw[k] = f[u * stride]; rw[k] = r[u * stride];
            }
#pragma unroll
            for (uint32_t k = 0; k < kFillBlock; ++k) prev = step(kForward ? done + k : N - 1u - done - k, fw[k], rw[k], prev);
        }
        for (; done < N; ++done) {
            const size_t u = kForward ? done : N - 1u - done;
            prev = step(u, f[u * stride], r[u * stride], prev);
        }
    }
    DXV_HD bool run()
    {
        pass<true>();
        pass<false>();
        return changed;
    }
};

// ---- write-back: one byte of the masks -> the bits of eight result bytes (what = 0: everything the flood did not reach, walls included;
// 1: the free voxels it did not reach) ----
DXV_HD uint32_t fill_result_byte(uint32_t free8, uint32_t reached8, int what) { return (what ? free8 : 0xffu) & ~reached8 & 0xffu; }
// ... as eight bytes of 0 / 1
DXV_HD uint64_t fill_spread_byte(uint32_t bits)
{
    const uint64_t own = ((uint64_t)bits * 0x0101010101010101ull) & 0x8040201008040201ull;     // byte k keeps bit k
    return ((own + 0x7f7f7f7f7f7f7f7full) >> 7) & 0x0101010101010101ull;
}

} // namespace dxv
