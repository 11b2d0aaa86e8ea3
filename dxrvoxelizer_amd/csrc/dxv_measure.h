// dxv_measure.h -- the integral measures of the components of a labelling (DESIGN.md §2 has the rule; include/dxv.h the record): what ONE RUN of
// set bits inside one word of the member mask (dxv_components.h: the fill's layout, bits behind a row's end 0) adds to its component.  All of it
// is exact integer arithmetic in 64 bits, and every measure is a SUM over the component's voxels or over cells each of which lies in exactly one
// component, so runs can be added in any order:
//   voxels, sum, sum2, prod   the moments of the voxel indices x0 .. x1 of the run at (y, z), in closed form: no loop over voxels
//   faces                     pairs (p, d), d one of the six axis steps, p + d a non-member or outside the grid: for each step the word of
//                             the neighbours at that step, bit for bit under the word itself (MeasRow: the x steps carry bit 63 / bit 0 of
//                             the words beside it), and a popcount of run & ~neighbours.  A row outside the grid is all clear.
//   euler, connectivity 6     v - e + f - c of the voxels, 6-adjacent pairs, axis-aligned 2 x 2 x 1 squares and 2 x 2 x 2 blocks inside the
//                             component; a cell is anchored at its LOWEST voxel, so a voxel has its three edges, three squares and one block
//                             towards +x, +y, +z: ANDs of the word with the +1 neighbours, a popcount under the run's bits.  Such a cell is
//                             6-connected: it lies in one component.
//   euler, connectivity 26    corners - edges + faces - cubes of the complex of closed unit cubes of the component.  A voxel p has 26 cells
//                             besides its cube, one per d in {-1, 0, 1}^3 \ 0 (a face for one non-zero axis, an edge for two, a corner for
//                             three); the voxels round that cell are p + s, s taking 0 or d per axis.  The cell is OWNED by the first member,
//                             in (z, y, x) order, among them: p owns it iff none of the p + s that precede p is a member, and p + s precedes
//                             p iff the most significant non-zero axis of s (z, then y, then x) is -1.  So every cell with a member round it
//                             is counted once, at a voxel of the one component that holds all the members round it (they are mutually
//                             26-adjacent).  An AND-NOT over shifted neighbour words, a popcount under the run's bits, sign (-1)^(3 - axes).
// No table is indexed by a lane's value, nothing goes to scratch memory.  No sum overflows for N <= kCompMaxN = 1624: sum2 < 1624^5 < 2^63.
// Everything here is __host__ __device__: measure.hip runs it on the GPU, tests/test_measure_rule.py compiles the same text for the CPU.
#pragma once
#include <stddef.h>
#include "dxv_types.h"
#include "dxv_solid.h"
#include "dxv_fill.h"
#include "dxv_components.h"

namespace dxv {

// one row of the table, 96 bytes, little endian (include/dxv.h)
struct MeasureRecord {
    uint64_t voxels, sum[3], sum2[3], prod[3], faces;
    int64_t euler;
};
static_assert(sizeof(MeasureRecord) == 96, "the measure's record is 96 bytes");
constexpr uint32_t kMeasureValues = 12;           // 64-bit words of a record, the order of its fields; euler by two's complement
enum { MEAS_VOXELS = 0, MEAS_SUM = 1, MEAS_SUM2 = 4, MEAS_PROD = 7, MEAS_FACES = 10, MEAS_EULER = 11 };

// a mask row as seen from one of its words: the word, and the voxels one step to the left and to the right of each of its bits
struct MeasRow {
    uint64_t at;            // bit b: voxel b of the word
    uint64_t lo;            // bit b: voxel b - 1 (bit 0: bit 63 of the word before)
    uint64_t hi;            // bit b: voxel b + 1 (bit 63: bit 0 of the word behind)
};
DXV_HD MeasRow meas_row(uint64_t prev, uint64_t cur, uint64_t next) { return {cur, (cur << 1) | (prev >> 63), (cur >> 1) | (next << 63)}; }
DXV_HD uint64_t meas_shifted(const MeasRow& r, int dx) { return dx < 0 ? r.lo : dx > 0 ? r.hi : r.at; }

// which of the nine rows (dz + 1) * 3 + (dy + 1) round a row a connectivity reads: all of them at 26; at 6 the row, its four face neighbours
// (faces) and (+1, +1) (the squares and blocks towards +y, +z)
DXV_HD bool meas_needs_row(uint32_t connectivity, int dy, int dz) { return connectivity == 26u || dy == 0 || dz == 0 || (dy == 1 && dz == 1); }

// rows[(dz + 1) * 3 + (dy + 1)]: the rows round word w of row (y, z); a row outside the grid, or one the connectivity does not read, is clear
DXV_HD void meas_load_rows(const uint64_t* mask, uint32_t N, uint32_t connectivity, uint32_t y, uint32_t z, uint32_t w, MeasRow* rows)
{
    const uint32_t W = fill_row_words(N);
#pragma unroll
    for (int k = 0; k < 9; ++k) {
        const int dy = k % 3 - 1, dz = k / 3 - 1;
        const int ny = (int)y + dy, nz = (int)z + dz;
        rows[k] = MeasRow{0ull, 0ull, 0ull};
        if (!meas_needs_row(connectivity, dy, dz) || ny < 0 || ny >= (int)N || nz < 0 || nz >= (int)N) continue;
        const uint64_t* r = mask + ((size_t)nz * N + (size_t)ny) * W;
        rows[k] = meas_row(w ? r[w - 1u] : 0ull, r[w], w + 1u < W ? r[w + 1u] : 0ull);
    }
}
DXV_HD const MeasRow& meas_at(const MeasRow* rows, int dy, int dz) { return rows[(dz + 1) * 3 + (dy + 1)]; }

// the members of the word that own their cell d at connectivity 26 (head comment)
DXV_HD uint64_t meas_owned(const MeasRow* rows, int dx, int dy, int dz)
{
    uint64_t before = 0;
#pragma unroll
    for (int k = 1; k < 8; ++k) {
        const int sx = (k & 1) ? dx : 0, sy = (k & 2) ? dy : 0, sz = (k & 4) ? dz : 0;
        if (((k & 1) && !dx) || ((k & 2) && !dy) || ((k & 4) && !dz)) continue;    // (this s has been taken with the bit clear)
        const bool precedes = sz ? sz < 0 : sy ? sy < 0 : sx < 0;
        if (precedes) before |= meas_shifted(meas_at(rows, sy, sz), sx);
    }
    return meas_at(rows, 0, 0).at & ~before;
}

// what a word's runs are counted under: the six face neighbours, and the cells its voxels bring with sign + and with sign -.  kConn = 26: eight
// corners and six faces +, twelve edges -, and -1 per voxel (its cube); kConn = 6: three squares +, three edges and a block -, +1 per voxel.
template <uint32_t kConn> struct MeasWord {
    static constexpr uint32_t kPlus = kConn == 26u ? 14u : 3u, kMinus = kConn == 26u ? 12u : 4u;
    uint64_t next[6];
    uint64_t plus[kPlus], minus[kMinus];
};

template <uint32_t kConn> DXV_HD void meas_word(const MeasRow* rows, MeasWord<kConn>& c)
{
    const MeasRow& m = meas_at(rows, 0, 0);
    c.next[0] = m.lo; c.next[1] = m.hi;
    c.next[2] = meas_at(rows, -1, 0).at; c.next[3] = meas_at(rows, 1, 0).at;
    c.next[4] = meas_at(rows, 0, -1).at; c.next[5] = meas_at(rows, 0, 1).at;
    if (kConn == 26u) {
        uint32_t p = 0, q = 0;
#pragma unroll
        for (int k = 0; k < 27; ++k) {
            const int dx = k % 3 - 1, dy = k / 3 % 3 - 1, dz = k / 9 - 1;
            const int axes = (dx != 0) + (dy != 0) + (dz != 0);
            if (!axes) continue;
            const uint64_t own = meas_owned(rows, dx, dy, dz);
            if (axes == 2) c.minus[q++] = own; else c.plus[p++] = own;
        }
    } else {
        const uint64_t x = m.hi, y = meas_at(rows, 1, 0).at, z = meas_at(rows, 0, 1).at;
        const uint64_t xy = meas_at(rows, 1, 0).hi, xz = meas_at(rows, 0, 1).hi, yz = meas_at(rows, 1, 1).at, xyz = meas_at(rows, 1, 1).hi;
        c.minus[0] = m.at & x; c.minus[1] = m.at & y; c.minus[2] = m.at & z;
        c.plus[0] = m.at & x & y & xy; c.plus[1] = m.at & y & z & yz; c.plus[2] = m.at & z & x & xz;
        c.minus[3] = c.plus[0] & z & xz & yz & xyz;
    }
}

// the bits s .. s + len - 1 (1 <= len, s + len <= 64)
DXV_HD uint64_t meas_run_bits(uint32_t s, uint32_t len) { return (len == 64u ? ~0ull : (1ull << len) - 1ull) << s; }
// 0^2 + 1^2 + .. + a^2
DXV_HD uint64_t meas_squares(uint64_t a) { return a * (a + 1ull) * (2ull * a + 1ull) / 6ull; }

// v[kMeasureValues]: what the run of the word's bits s .. s + len - 1, the voxels x0 .. x0 + len - 1 of row (y, z), adds to its component
template <uint32_t kConn> DXV_HD void meas_run(const MeasWord<kConn>& c, uint32_t s, uint32_t len, uint32_t x0, uint32_t y, uint32_t z, uint64_t* v)
{
    const uint64_t n = len, a = x0, b = (uint64_t)x0 + len - 1ull;
    const uint64_t sx = n * (a + b) / 2ull;                             // (n and a + b are not both odd)
    v[MEAS_VOXELS] = n;
    v[MEAS_SUM] = sx; v[MEAS_SUM + 1] = n * y; v[MEAS_SUM + 2] = n * z;
    v[MEAS_SUM2] = meas_squares(b) - (a ? meas_squares(a - 1ull) : 0ull); v[MEAS_SUM2 + 1] = n * y * y; v[MEAS_SUM2 + 2] = n * z * z;
    v[MEAS_PROD] = sx * y; v[MEAS_PROD + 1] = n * y * z; v[MEAS_PROD + 2] = sx * z;
    const uint64_t run = meas_run_bits(s, len);
    uint32_t faces = 0, plus = 0, minus = 0;
#pragma unroll
    for (uint32_t k = 0; k < 6u; ++k) faces += solid_popc(run & ~c.next[k]);
#pragma unroll
    for (uint32_t k = 0; k < MeasWord<kConn>::kPlus; ++k) plus += solid_popc(run & c.plus[k]);
#pragma unroll
    for (uint32_t k = 0; k < MeasWord<kConn>::kMinus; ++k) minus += solid_popc(run & c.minus[k]);
    v[MEAS_FACES] = faces;
    const int64_t own = kConn == 26u ? -(int64_t)len : (int64_t)len;
    v[MEAS_EULER] = (uint64_t)(own + (int64_t)plus - (int64_t)minus);
}

} // namespace dxv
