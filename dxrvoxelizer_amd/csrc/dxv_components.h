// dxv_components.h -- the connected components of a whole N^3 grid (DESIGN.md §2 has the rule) on BITS and by UNION-FIND.  The members --
// the solid voxels, or the empty ones -- are one bit per voxel in the fill's mask layout (dxv_fill.h: rows of fill_row_words(N) 64-bit words,
// bit x % 64 of word x / 64, the bits behind a row's end 0).  parent[] is the label buffer itself, one uint32 per voxel at its linear index
// (iz * N + iy) * N + ix:
//   init      parent[p] = the linear index of the start of p's run of set bits inside its own word (bit operations on the word: adjacency
//             along x inside a word costs no union), kCompNone for a voxel that is no member;
//   merge     one mask word at a time: bit 0 with bit 63 of the word before it in the row, and the word's members with the members of
//             the EARLIER neighbour rows -- 2 rows for connectivity 6, 4 rows with x offsets -1, 0, +1 for 26.  A pair (p, q) at an offset
//             needs no union when another pair stands for it: at x offset 0 only the first bit of each run of m & n unites (the pair one
//             step to the left joins the same two runs); at x offset -1 only where p starts a run of m and q ends a run of n, at +1 only
//             where p ends a run and q starts one -- every other diagonal pair has a pair of offset 0 beside it that joins the same runs;
//   compress  parent[p] = the root of p, which is the smallest index of its component: first(C).
// comp_union hooks the LARGER root under the SMALLER with an atomic minimum, so parent[i] <= i always holds and only ever falls: every loop
// here ends because an index strictly falls (comp_find: a; comp_union: the larger root).  What holds at every instant, with any number of
// lanes in these routines at once: an entry only ever points at a voxel of its own component (a hook joins two voxels the rule joins, a
// lowering replaces a parent by something reached from it).  What does NOT hold at every instant is that the trees only grow together:
// when comp_union finds a already hooked (old != a) and b < old, its minimum has moved parent[a] from old to b BEFORE old's set and b's are
// joined, and for that moment a's subtree hangs under a tree that old's is not yet part of.  The lane that did it holds the pair (old, b)
// and goes on with it at once; it waits for nobody, and it returns only when a hook of its own succeeded or it found its two voxels under
// one root.  So the claim is about the END: when every lane has returned no pair is held any more, and the two voxels of every union that
// was asked for stand under one root.  The result is read only then (components.hip: behind the kernel boundary).  This is the union of the
// published GPU labelling algorithms (Komura 2015; Playne and Hawick 2018).
// The parent array is reached through a policy -- load(i), lower(i, v) = atomic min returning the old value -- so that components.hip runs
// this text with agent-scope atomics and tests/test_components_rule.py runs the same text on the CPU with plain accesses.
// Everything here is __host__ __device__.
#pragma once
#include <stddef.h>
#include "dxv_types.h"
#include "dxv_solid.h"
#include "dxv_fill.h"

namespace dxv {

constexpr uint32_t kCompNone = 0xffffffffu;       // parent of a voxel that is no member (no member's index: N <= 1624, N^3 < 2^32)
constexpr uint32_t kCompMaxN = 1624;              // 1624^3 < 2^32 < 1626^3 and N is even: labels and linear indices fit a uint32
enum { COMP_SOLID = 0, COMP_EMPTY = 1 };          // DXV_COMP_*
enum { COMP_SELECT_LARGEST = 0, COMP_SELECT_MIN_VOXELS = 1, COMP_SELECT_BORDER = 2 };   // DXV_SELECT_*

// one row of the table, 24 bytes, little endian (include/dxv.h)
struct CompRecord {
    uint32_t first, voxels;
    uint16_t lo[3], hi[3];
    uint32_t flags;
};
static_assert(sizeof(CompRecord) == 24, "the table's record is 24 bytes");

// what the stats pass gathers per component with 32-bit integer atomics before the table is packed
using CompStats = BoxStats;

DXV_HD uint32_t comp_ctz(uint64_t v)              // v != 0
{
#if defined(__HIP_DEVICE_COMPILE__)
    return (uint32_t)__ffsll((unsigned long long)v) - 1u;
#else
    return (uint32_t)__builtin_ctzll(v);
#endif
}
DXV_HD uint32_t comp_clz(uint64_t v)              // v != 0
{
#if defined(__HIP_DEVICE_COMPILE__)
    return (uint32_t)__clzll((long long)v);
#else
    return (uint32_t)__builtin_clzll(v);
#endif
}
DXV_HD uint32_t comp_popc(uint64_t v) { return solid_popc(v); }

// ---- pack: eight voxels -> one byte of the member mask.  j: the byte's place in its row (voxels 8j .. 8j+7) ----
DXV_HD uint32_t comp_member_byte(const uint8_t* row, uint32_t N, uint32_t j, int of)
{
    const uint32_t left = N - 8u * j, valid = left >= 8u ? 0xffu : (1u << left) - 1u;
    const uint32_t s = solid_bits(row + 8u * j, left);
    return (of == COMP_EMPTY ? ~s : s) & valid;
}
// ... from eight bytes loaded as one word (N % 8 == 0)
DXV_HD uint32_t comp_member_byte(uint64_t eight, int of) { return (of == COMP_EMPTY ? ~solid_bits(eight) : solid_bits(eight)) & 0xffu; }

// ---- init: the start of the run of set bits of m that holds bit b (m has bit b) ----
DXV_HD uint32_t comp_run_start(uint64_t m, uint32_t b)
{
    const uint64_t zeros = ~m & ((1ull << b) - 1ull);                   // the clear bits below b: the run starts behind the highest of them
    return zeros ? 64u - comp_clz(zeros) : 0u;
}
DXV_HD uint32_t comp_init_parent(const uint64_t* mask, uint32_t N, uint32_t p)
{
    const uint32_t row = p / N, x = p - row * N;
    const uint64_t m = mask[(size_t)row * fill_row_words(N) + (x >> 6)];
    if (!(m >> (x & 63u) & 1ull)) return kCompNone;
    return p - (x & 63u) + comp_run_start(m, x & 63u);
}

// ---- union-find.  P: load(i) and lower(i, v) = { old = parent[i]; parent[i] = min(old, v); return old; } ----
// the root of a; on the way every visited entry is lowered to what its parent pointed at when read (a voxel of the same component with a
// smaller index: a valid parent, see the head comment).  a strictly falls.
template <class P> DXV_HD uint32_t comp_find(P& par, uint32_t a)
{
    for (;;) {
        const uint32_t pa = par.load(a);
        if (pa == a) return a;
        const uint32_t ga = par.load(pa);                               // ga <= pa < a
        if (ga < pa) (void)par.lower(a, ga);
        a = ga;
    }
}
// the root of a without a write (the compress pass, behind the merge kernel: the trees are final, every entry it reads is an ancestor of a,
// whoever wrote it)
template <class P> DXV_HD uint32_t comp_root(P& par, uint32_t a)
{
    for (;;) {
        const uint32_t pa = par.load(a);
        if (pa == a) return a;
        a = pa;
    }
}
// one component out of a's and b's.  Lock-free: nobody waits; a pass ends the loop or replaces the larger root by a strictly smaller index.
template <class P> DXV_HD void comp_union(P& par, uint32_t a, uint32_t b)
{
    for (;;) {
        a = comp_find(par, a);
        b = comp_find(par, b);
        if (a == b) return;
        if (a < b) { const uint32_t t = a; a = b; b = t; }              // a: the larger root, hooked under the smaller
        const uint32_t old = par.lower(a, b);
        if (old == a) return;                                           // a was still a root
        a = old;                                                        // somebody hooked a first, under old < a; a now points at min(old, b), and old's
                                                                        // set and b's are still to join: this lane's job, at once (head comment)
    }
}

// the earlier neighbour rows of a row: k-th of comp_rows(connectivity) as (dy, dz)
DXV_HD uint32_t comp_rows(uint32_t connectivity) { return connectivity == 26u ? 4u : 2u; }
DXV_HD void comp_row_offset(uint32_t connectivity, uint32_t k, int& dy, int& dz)
{
    dz = k ? -1 : 0;                                                    // 6: (-1, 0), (0, -1);  26: (-1, 0), (-1, -1), (0, -1), (+1, -1)
    dy = k ? (connectivity == 26u ? (int)k - 2 : 0) : -1;
}

// ---- merge: the unions of word w of row (iy, iz) ----
template <class P> DXV_HD void comp_merge_word(P& par, const uint64_t* mask, uint32_t N, uint32_t connectivity, uint32_t iy, uint32_t iz, uint32_t w)
{
    const uint32_t W = fill_row_words(N);
    const uint64_t* mr = mask + ((size_t)iz * N + iy) * W;
    const uint64_t m = mr[w];
    if (!m) return;
    const uint32_t base = (iz * N + iy) * N + 64u * w;                  // the linear index of the word's bit 0
    const uint64_t mPrev = w ? mr[w - 1u] : 0ull, mNext = w + 1u < W ? mr[w + 1u] : 0ull;
    if ((m & 1ull) && (mPrev >> 63)) comp_union(par, base, base - 1u);
    for (uint32_t k = 0; k < comp_rows(connectivity); ++k) {
        int dy, dz;
        comp_row_offset(connectivity, k, dy, dz);
        const int ny = (int)iy + dy, nz = (int)iz + dz;
        if (ny < 0 || ny >= (int)N || nz < 0) continue;
        const uint64_t* nr = mask + ((size_t)nz * N + (size_t)ny) * W;
        const uint32_t nbase = ((uint32_t)nz * N + (uint32_t)ny) * N + 64u * w;
        const uint64_t n = nr[w], nPrev = w ? nr[w - 1u] : 0ull, nNext = w + 1u < W ? nr[w + 1u] : 0ull;
        const uint64_t both = m & n;
        uint64_t c = both & ~(both << 1 | (mPrev & nPrev) >> 63);       // x offset 0: the first bit of each run of m & n, runs carried over from the word before
        while (c) {
            const uint32_t s = comp_ctz(c);
            c &= c - 1ull;
            comp_union(par, base + s, nbase + s);
        }
        if (connectivity != 26u) continue;
        c = m & ~(m << 1 | mPrev >> 63) & (n << 1 | nPrev >> 63) & ~n;  // x offset -1: p starts a run of m, q = x - 1 ends a run of n
        while (c) {
            const uint32_t s = comp_ctz(c);
            c &= c - 1ull;
            comp_union(par, base + s, nbase + s - 1u);
        }
        c = m & ~(m >> 1 | mNext << 63) & (n >> 1 | nNext << 63) & ~n;  // x offset +1: p ends a run of m, q = x + 1 starts a run of n
        while (c) {
            const uint32_t s = comp_ctz(c);
            c &= c - 1ull;
            comp_union(par, base + s, nbase + s + 1u);
        }
    }
}

// ---- number: the rank of root r among the roots, from one bit per voxel in LINEAR order and the roots in front of every 64 voxels ----
DXV_HD uint32_t comp_rank(const uint64_t* rootMask, const uint32_t* bases, uint32_t r)
{
    return bases[r >> 6] + comp_popc(rootMask[r >> 6] & ((1ull << (r & 63u)) - 1ull));
}

// ---- stats: the next run of set bits of m (m != 0), taken out of it: bits s .. s + len - 1 ----
DXV_HD void comp_take_run(uint64_t& m, uint32_t& s, uint32_t& len)
{
    s = comp_ctz(m);
    const uint64_t rest = ~(m >> s);                                    // (s > 0: bit 64 - s and above are set, a run up to bit 63 ends there)
    len = rest ? comp_ctz(rest) : 64u;
    m &= len == 64u ? 0ull : ~(((1ull << len) - 1ull) << s);
}
DXV_HD uint32_t comp_run_flags(uint32_t N, uint32_t x0, uint32_t x1, uint32_t y, uint32_t z)
{
    return (x0 == 0u || x1 == N - 1u || y == 0u || y == N - 1u || z == 0u || z == N - 1u) ? 1u : 0u;
}
DXV_HD CompRecord comp_record(uint32_t first, const CompStats& s)
{
    CompRecord r;
    r.first = first; r.voxels = s.voxels; r.flags = s.flags;
    for (int a = 0; a < 3; ++a) { r.lo[a] = (uint16_t)s.lo[a]; r.hi[a] = (uint16_t)s.hi[a]; }
    return r;
}

// ---- select ----
// the order "most voxels, ties to the smaller number" as one 64-bit maximum; number = 1 .. K
DXV_HD unsigned long long comp_best_key(uint32_t voxels, uint32_t number) { return (unsigned long long)voxels << 32 | (uint32_t)~number; }
DXV_HD uint32_t comp_best_number(unsigned long long key) { return ~(uint32_t)key; }
// whether component `number` is kept; best: the maximum of comp_best_key over the table (DXV_SELECT_LARGEST reads nothing else)
DXV_HD bool comp_keep(int rule, uint32_t arg, uint32_t number, uint32_t voxels, uint32_t flags, unsigned long long best)
{
    if (rule == COMP_SELECT_LARGEST) return number == comp_best_number(best);
    if (rule == COMP_SELECT_MIN_VOXELS) return voxels >= arg;
    return (flags & 1u) != 0u;
}

// ---- what components.hip's launches work on: labels = N^3 uint32 and table = 24 K bytes are the caller's, stats = K CompStats of work ----
struct CompParams {
    const uint8_t* grid;    // N^3 bytes, element (iz * N + iy) * N + ix; a voxel is solid iff its byte is non-zero
    uint32_t N;
    int of;                 // DXV_COMP_SOLID / DXV_COMP_EMPTY
    uint32_t connectivity;  // 6 / 26
    uint32_t* labels;       // parent during the build, then the labels
    uint64_t* mask;         // comp_carve fills these five
    uint64_t* rootMask;
    uint32_t* bases;
    unsigned long long* sums;
    unsigned long long* total;    // K
    CompStats* stats;
    CompRecord* table;
};
inline size_t comp_linear_words(uint32_t N) { return ((size_t)N * N * N + 63u) / 64u; }
// scratch of one build: the member mask, the root bits and the roots in front of every 64 voxels, the scan's block sums, the total
inline void comp_carve(Carve& c, uint32_t N, CompParams& p)
{
    const size_t words = comp_linear_words(N);
    p.N = N;
    p.mask = c.take<uint64_t>(fill_mask_words(N));
    p.rootMask = c.take<uint64_t>(words);
    p.bases = c.take<uint32_t>(words);
    p.sums = c.take<unsigned long long>(scan_blocks(words));
    p.total = c.take<unsigned long long>(1);
}
inline size_t comp_scratch_bytes(uint32_t N) { return carved_bytes<CompParams>(comp_carve, N); }

// work of dxv_components_select: {kept, dropped, voxels changed, the maximum of comp_best_key}, then K keep flags
struct CompSelectWork { unsigned long long* counters; uint8_t* keep; };
inline void comp_select_carve(Carve& c, uint32_t K, CompSelectWork& w)
{
    w.counters = c.take<unsigned long long>(4);
    w.keep = c.take<uint8_t>(K);
}
inline size_t comp_select_bytes(uint32_t K) { return carved_bytes<CompSelectWork>(comp_select_carve, K); }

} // namespace dxv
