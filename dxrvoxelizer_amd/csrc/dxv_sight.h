// dxv_sight.h -- the line-of-sight map of a grid: with M the members (the solid voxels, or the empty ones) and d one of the 26
// lattice directions {-1, 0, 1}^3 \ {0}, bit b(d) = (dz + 1) * 9 + (dy + 1) * 3 + (dx + 1) of a uint32 (13, the zero vector, is never set; d and
// -d have bits b and 26 - b; the 13 axes are the pairs with b > 13, axis a = b - 14),
//     V_d(c) = M(c) and (c - d outside the grid or V_d(c - d))
// -- a member is seen along d when a ray that enters the grid travelling in direction d reaches it through members only.  The map word of a
// voxel is the OR of the bits of the requested directions along which it is seen, 0 on a voxel that is no member.  On BITS: M and one plane
// V_d per requested direction in the fill's layout (dxv_fill.h: rows of fill_row_words(N) 64-bit words, bit x % 64 of word x / 64, the bits
// behind the row's end 0, word (iz * N + iy) * W + w).
// The sweep of a direction runs along z where dz != 0, else along y where dy != 0, else along x.  Along z or y a LINE FAMILY is the set of
// lines that share a row in every plane of the sweep: its words keep their place w in the row, the row moves by the sheared coordinate's step
// (dy under a z sweep) and the bits by dx.  A family is named by the row it would hold at step 0, rows outside the grid included: 2N - 1
// families where the row moves, N where it does not; outside the grid a family's state is all ones.  One step of one word:
//     V' = M & V                         dx = 0
//     V' = M & ((V << 1) | in)           dx = +1: in = the top bit of the word below as it stood BEFORE the step; 1 at the row's start
//     V' = M & ((V >> 1) | in << 63)     dx = -1: in = the bottom bit of the word above; at the row's end a 1 at bit (N - 1) % 64
// Along x alone a row is scanned in itself (sight_row_x).  Every word of a plane is written exactly once, zeros included.
// The tally comes from the words: popcounts for `seen` and `neither`, a bit-sliced counter over the planes for `count`.  Sums of integers: the
// order of the combines does not matter.  Everything here is __host__ __device__: sight.hip runs it on the GPU,
// tests/hostcheck/sight_check.cpp word by word on the CPU.  Two things the host alone calls: sight_map_word, which composes a voxel's word
// from all 27 planes' words with sight_map_bit -- the device calls sight_map_bit itself, once per REQUESTED plane, on the word a lane hands
// round its wave --, and sight_tally_combine, where the device adds a wave's shares by shuffles and a workgroup's by atomics.
#pragma once
#include "dxv_fill.h"
#include "dxv_thickness.h"

namespace dxv {

constexpr uint32_t kSightMaxN = kThickMaxN;       // the map is 4 N^3 bytes and a voxel's linear index fits the word other maps use
constexpr uint32_t kSightBits = 27;               // bits of a map word, the never-set bit 13 among them
constexpr uint32_t kSightAxes = 13;
constexpr uint32_t kSightAll = 0x07FFDFFFu;       // DXV_SIGHT_ALL
constexpr uint32_t kSightBlock = 8;               // steps of a sweep whose loads are issued together, in front of the chain through them (as kFillBlock)
constexpr uint32_t kSightMaxGroup = 16;           // lanes of a row group at the most: fill_row_words(kSightMaxN)
constexpr uint32_t kSightTallyWords = 1u + kSightBits + kSightAxes + kSightBits;       // 68

DXV_HD uint32_t sight_bit(int dx, int dy, int dz) { return (uint32_t)((dz + 1) * 9 + (dy + 1) * 3 + (dx + 1)); }
DXV_HD int sight_dx(uint32_t b) { return (int)(b % 3u) - 1; }
DXV_HD int sight_dy(uint32_t b) { return (int)(b / 3u % 3u) - 1; }
DXV_HD int sight_dz(uint32_t b) { return (int)(b / 9u) - 1; }
DXV_HD bool sight_directions_valid(uint32_t directions) { return directions != 0u && !(directions & ~kSightAll); }
DXV_HD bool sight_valid(uint32_t N, int of, uint32_t directions)
{
    return N >= 2u && N <= kSightMaxN && !(N & 1u) && (of == THICK_SOLID || of == THICK_EMPTY) && sight_directions_valid(directions);
}
DXV_HD uint32_t sight_popc(uint64_t v) { return solid_popc(v); }
// the lowest set bit's number (v != 0)
DXV_HD uint32_t sight_lowest(uint32_t v)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return (uint32_t)__ffs((int)v) - 1u;
#else
    return (uint32_t)__builtin_ctz(v);
#endif
}
// the bits of word w of a row that lie inside the grid
DXV_HD uint64_t sight_inside(uint32_t N, uint32_t w)
{
    const uint32_t rest = N - 64u * w;
    return rest >= 64u ? ~0ull : (1ull << rest) - 1ull;
}

// ---- pack: eight voxels -> one byte of M (dxv_morph.h's member byte: the complement inside the grid for the empty kind) ----
DXV_HD uint32_t sight_member_byte(const uint8_t* row, uint32_t N, uint32_t j, int of)
{
    const uint32_t left = N - 8u * j, valid = left >= 8u ? 0xffu : (1u << left) - 1u, s = solid_bits(row + 8u * j, left);
    return (of == THICK_EMPTY ? ~s : s) & valid;
}
DXV_HD uint32_t sight_member_byte(uint64_t eight, int of) { return (of == THICK_EMPTY ? ~solid_bits(eight) : solid_bits(eight)) & 0xffu; }

// ---- the sweep of one direction ----
// lanes side by side that hold the words of one row: the next power of two >= W, or `atLeast` (option sightgroup) where that is more
DXV_HD uint32_t sight_group(uint32_t W, uint32_t atLeast)
{
    uint32_t G = 1;
    while (G < W || G < atLeast) G <<= 1;
    return G;
}
// axis: 0 = the rows scanned in themselves, 1 = planes of constant y, 2 = of constant z.  step: +1 the sweep runs up its axis, -1 down.
// shear: what the family's row moves by per step (dy under a z sweep).  rowStride, stepStride: words between rows of a family, between steps.
struct SightSweep { int axis, step, shear, dx; uint32_t families; size_t rowStride, stepStride; };
DXV_HD SightSweep sight_sweep(uint32_t b, uint32_t N)
{
    const int dx = sight_dx(b), dy = sight_dy(b), dz = sight_dz(b);
    const size_t W = fill_row_words(N);
    if (dz) return SightSweep{2, dz, dy, dx, dy ? 2u * N - 1u : N, W, W * N};
    if (dy) return SightSweep{1, dy, 0, dx, N, W * N, W};
    return SightSweep{0, dx, 0, dx, N * N, W, 0};
}
// the place along the sweep's axis of step k, and the row family f holds there (outside [0, N): the family is outside the grid)
DXV_HD uint32_t sight_step_at(const SightSweep& s, uint32_t N, uint32_t k) { return s.step > 0 ? k : N - 1u - k; }
DXV_HD int32_t sight_row_at(const SightSweep& s, uint32_t N, uint32_t f, uint32_t k)
{
    return s.shear > 0 ? (int32_t)f - (int32_t)(N - 1u) + (int32_t)k : s.shear < 0 ? (int32_t)f - (int32_t)k : (int32_t)f;
}
// what a word hands to its neighbour in the row: its top bit for dx = +1, its bottom bit for dx = -1
DXV_HD uint32_t sight_carry(uint64_t V, int dx) { return (uint32_t)(dx > 0 ? V >> 63 : V & 1ull); }
// one step of word w of a row of W: M the members there, V the family's word one step back, in the neighbour's carry from one step back
DXV_HD uint64_t sight_step(uint64_t M, uint64_t V, uint32_t in, int dx, uint32_t N, uint32_t w, uint32_t W)
{
    if (dx == 0) return M & V;
    if (dx > 0) return M & ((V << 1) | (w == 0u ? 1ull : (uint64_t)in));
    return M & ((V >> 1) | (w + 1u == W ? 1ull << ((N - 1u) & 63u) : (uint64_t)in << 63));
}
// along x alone: the members of a row below its first non-member (dx = +1), above its last (dx = -1)
DXV_HD void sight_row_x(const uint64_t* m, uint64_t* v, uint32_t N, uint32_t W, int dx)
{
    bool open = true;
    for (uint32_t i = 0; i < W; ++i) {
        const uint32_t w = dx > 0 ? i : W - 1u - i;
        const uint64_t stop = ~m[w] & sight_inside(N, w);                // the non-members of the word
        uint64_t seen = 0;
        if (open) {
            if (!stop) seen = m[w];
            else if (dx > 0) seen = m[w] & ((stop & (0ull - stop)) - 1ull);
            else {
                const uint64_t r = fill_reverse(stop);
                seen = m[w] & fill_reverse((r & (0ull - r)) - 1ull);
            }
            open = !stop;
        }
        v[w] = seen;
    }
}

// ---- compose: the map word of voxel x % 64 of a mask word from the planes' words there (v[b]: 0 for a direction not asked for) ----
// ... one plane's share of it: bit x of the plane's word V as bit b of the map word
DXV_HD uint32_t sight_map_bit(uint64_t V, uint32_t x, uint32_t b) { return (uint32_t)((V >> x) & 1ull) << b; }
DXV_HD uint32_t sight_map_word(const uint64_t* v, uint32_t bit)
{
    uint32_t word = 0;
#pragma unroll
    for (uint32_t b = 0; b < kSightBits; ++b) word |= sight_map_bit(v[b], bit, b);
    return word;
}

// ---- the tally: 68 integers.  T: uint64 for the record, uint32 for a thread's share of it ----
template <class T> struct SightTallyOf { T members, seen[kSightBits], neither[kSightAxes], count[kSightBits]; };
using SightTally = SightTallyOf<unsigned long long>;
static_assert(sizeof(SightTally) == kSightTallyWords * 8u, "the tally is 68 words");
template <class T, class U> DXV_HD void sight_tally_combine(SightTallyOf<T>& a, const SightTallyOf<U>& b)
{
    a.members += b.members;
    for (uint32_t k = 0; k < kSightBits; ++k) { a.seen[k] += b.seen[k]; a.count[k] += b.count[k]; }
    for (uint32_t k = 0; k < kSightAxes; ++k) a.neither[k] += b.neither[k];
}
// one mask word M and its planes' words (v[b]: 0 for a direction not asked for).  count: the planes are added into a counter of five bit
// slices, c[j] bit j of "the requested directions this voxel is seen along"; the members whose counter reads k are those of count[k].
template <class T> DXV_HD void sight_tally_word(SightTallyOf<T>& t, uint64_t M, const uint64_t* v, uint32_t directions)
{
    t.members += (T)sight_popc(M);
    uint64_t c[5] = {0, 0, 0, 0, 0};
#pragma unroll
    for (uint32_t b = 0; b < kSightBits; ++b) {
        if (!(directions >> b & 1u)) continue;
        t.seen[b] += (T)sight_popc(v[b]);
        if (b > 13u && (directions >> (26u - b) & 1u)) t.neither[b - 14u] += (T)sight_popc(M & ~v[b] & ~v[26u - b]);
        uint64_t carry = v[b];
#pragma unroll
        for (uint32_t j = 0; j < 5u; ++j) {
            const uint64_t up = c[j] & carry;
            c[j] ^= carry;
            carry = up;
        }
    }
#pragma unroll
    for (uint32_t k = 0; k < kSightBits; ++k) {
        uint64_t is = M;
#pragma unroll
        for (uint32_t j = 0; j < 5u; ++j) is &= (k >> j & 1u) ? c[j] : ~c[j];
        t.count[k] += (T)sight_popc(is);
    }
}

// ---- the edit: a member whose map word shares no bit with `directions` changes kind -- an empty member becomes the byte the fill writes
// for solid, a solid member 0 ----
DXV_HD bool sight_fill_changes(uint8_t voxel, uint32_t word, int of, uint32_t directions)
{
    return (of == THICK_EMPTY ? !solid(voxel) : solid(voxel)) && !(word & directions);
}
DXV_HD uint8_t sight_fill_byte(int of) { return of == THICK_EMPTY ? (uint8_t)1 : (uint8_t)0; }

// ---- scratch of one call: the tally's words, the member mask, one plane per requested direction ----
struct SightScratch { unsigned long long* tally; uint64_t *mask, *planes; };
inline void sight_carve(Carve& c, uint32_t N, uint32_t directions, SightScratch& l)
{
    l.tally = c.take<unsigned long long>(kSightTallyWords);
    l.mask = c.take<uint64_t>(fill_mask_words(N));
    l.planes = c.take<uint64_t>(fill_mask_words(N) * sight_popc(directions));
}
inline size_t sight_scratch_bytes(uint32_t N, uint32_t directions) { return carved_bytes<SightScratch>(sight_carve, N, directions); }

} // namespace dxv
