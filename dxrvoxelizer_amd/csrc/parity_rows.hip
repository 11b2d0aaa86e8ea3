// parity_rows.hip -- the parity rule's row kernel and its launch.
#include "dxv_device.h"
#include "dxv_trace.h"
#include "dxv_dirmap.h"

namespace dxv {

// ---------------------------------------------------------------------------------------------
// Parity mode, row kernel: one wavefront per run of 64*CH voxels of one grid row.  The tree walk
// is wave-uniform (it depends on the row and the run's left end only): node and triangle records
// arrive through the scalar cache into SGPRs, the stack is one LDS column per wave, branches are
// scalar.  Lanes only diverge in data: lane l owns voxels x0 + 64 c + l (c < CH) and evaluates
// parity_row_voxel for them.  Same per-voxel results as k_voxelize<..., MODE 1> (tests), an
// order of magnitude fewer node visits.
// ---------------------------------------------------------------------------------------------
#if defined(__HIP_DEVICE_COMPILE__)
__device__ __forceinline__ TriPos load_tri_scalar(const TriPos* tris, int32_t uniformLeaf)
{
    const char* p = reinterpret_cast<const char*>(tris) + (uint64_t)(uint32_t)uniformLeaf * 48u;
    uint64_t w0, w1, w2, w3, w4, w5;
    asm volatile("s_load_dwordx2 %0, %6, 0x0\n\ts_load_dwordx2 %1, %6, 0x8\n\ts_load_dwordx2 %2, %6, 0x10\n\t"
                 "s_load_dwordx2 %3, %6, 0x18\n\ts_load_dwordx2 %4, %6, 0x20\n\ts_load_dwordx2 %5, %6, 0x28\n\t"
                 "s_waitcnt lgkmcnt(0)"
                 : "=&s"(w0), "=&s"(w1), "=&s"(w2), "=&s"(w3), "=&s"(w4), "=&s"(w5) : "s"(p) : "memory");
    auto lo = [](uint64_t v) { return __builtin_bit_cast(float, (uint32_t)v); };
    auto hi = [](uint64_t v) { return __builtin_bit_cast(float, (uint32_t)(v >> 32)); };
    TriPos t;
    t.v0 = F4{lo(w0), hi(w0), lo(w1), hi(w1)};
    t.v1 = F4{lo(w2), hi(w2), lo(w3), hi(w3)};
    t.v2 = F4{lo(w4), hi(w4), lo(w5), hi(w5)};
    return t;
}

struct WaveStack {
    int32_t* base;   // LDS, one column per wave
    __device__ __forceinline__ void push(int& sp, int32_t v) { base[sp++] = v; }
    __device__ __forceinline__ int32_t pop(int& sp) { return __builtin_amdgcn_readfirstlane(base[--sp]); }
};
#endif

// RB = rows per side of the block of grid rows a wave owns: 1 (one row), 2 or 4.  The RB x RB rows
// share one walk over the union of their y/z: up to 2.7x faster where triangles span several
// voxels, slower where they are voxel sized (every visited triangle is set up once per row it
// might cross) -- the launcher decides by the mean triangle extent.
// WIDE: the walk takes the four-box nodes (Node64) -- half as many dependent scalar fetches, which is
// what the walk waits on (triangle arithmetic is 6 % of the kernel).
// LISTS (RB = 1): the candidates of a row come from the row lists of the parity rule (parity_lists.hip) -- one cell, then the
// triangles of its list four at a time -- instead of from a walk of the tree.
template <int CH, int RB, bool WIDE, bool LISTS = false>
__global__ __launch_bounds__(64, RB == 1 ? 8 : 6) void k_parity_rows(VoxelizeParams p)   // <= 64 / 80 VGPRs
{
#if defined(__HIP_DEVICE_COMPILE__)   // (the host pass only needs the stub: the body uses SGPR inline asm)
    static_assert(RB == 1 || RB == 2 || RB == 4, "1, 2 x 2 or 4 x 4 rows");
    constexpr int ROWS = RB * RB, WORDS = (ROWS * CH + 31) / 32;
    static_assert(32 % CH == 0, "a row's parity bits do not straddle registers");
    __shared__ int32_t stack[64];
    const uint32_t N = p.N;
    const uint32_t segLen = 64u * CH, nseg = (N + segLen - 1) / segLen;
    // blocks of RB x RB rows (y, z); rows past the end of the grid or slab repeat the last one
    // (same values written twice)
    const uint32_t by = (N + RB - 1u) / RB, bz = (p.nz + RB - 1u) / RB;
    const uint32_t nblocks = by * bz, nwaves = nblocks * nseg;
    const uint32_t rb = p.regionBits;
    const uint32_t j = blockIdx.x >> 3;
    const uint32_t lin = ((((j >> rb) << 3) | (blockIdx.x & 7u)) << rb) | (j & ((1u << rb) - 1u));
    if (lin >= nwaves) return;
    const uint32_t seg = lin % nseg;
    uint32_t blk = lin / nseg, biy, blz;
    constexpr uint32_t TS = RB == 4 ? 4u : 8u / RB, TB = RB == 1 ? 3u : 2u;   // 8 x 8 (16 x 16) rows per tile: neighbours share tree paths
    if (!(by & (TS - 1u)) && !(bz & (TS - 1u))) {
        const uint32_t tile = blk >> (2u * TB), in = blk & (TS * TS - 1u), tx = by >> TB;
        biy = (tile % tx) * TS + (in & (TS - 1u));
        blz = (tile / tx) * TS + (in >> TB);
    } else { biy = blk % by; blz = blk / by; }
    const uint32_t lane = threadIdx.x, x0 = seg * segLen;

    uint32_t iy[RB], lz[RB];
    float oy[RB], oz[RB], oxMin = 0.0f, t0, t1;
#pragma unroll
    for (int k = 0; k < RB; ++k) {
        iy[k] = biy * RB + k < N ? biy * RB + k : N - 1u;
        lz[k] = blz * RB + k < p.nz ? blz * RB + k : p.nz - 1u;
        const uint32_t iz = global_slice(p.z0, p.nz, p.zBlock, p.zShift, p.zPeriod, lz[k]);
        ray_origin(N, x0, iy[k], iz, oxMin, oy[k], t0);
        ray_origin(N, x0, iy[0], iz, t0, t1, oz[k]);
    }
    float ox[CH];
#pragma unroll
    for (int c = 0; c < CH; ++c) ray_origin(N, x0 + 64u * c + lane, iy[0], p.z0, ox[c], t0, t1);
    // lane r < ROWS carries the origin of row r = ry + RB * rz (the other lanes repeat rows; RB > 1 only)
    float oyLane = oy[0], ozLane = oz[0];
#pragma unroll
    for (int k = 1; k < RB; ++k) {
        if ((lane % ROWS) % RB == (uint32_t)k) oyLane = oy[k];
        if ((lane % ROWS) / RB == (uint32_t)k) ozLane = oz[k];
    }
    uint32_t bits[WORDS];                              // parity of voxel (row r = ry + RB * rz, run c) in bit r * CH + c
#pragma unroll
    for (int w = 0; w < WORDS; ++w) bits[w] = 0;
    float ylo = oy[0], yhi = oy[0], zlo = oz[0], zhi = oz[0];
#pragma unroll
    for (int k = 1; k < RB; ++k) { ylo = min_(ylo, oy[k]); yhi = max_(yhi, oy[k]); zlo = min_(zlo, oz[k]); zhi = max_(zhi, oz[k]); }
    const SceneView& sc = p.scene;
    if (sc.rootLo[1] <= yhi && ylo <= sc.rootHi[1] && sc.rootLo[2] <= zhi && zlo <= sc.rootHi[2] && sc.rootHi[0] >= oxMin) {
        WaveStack stk{stack};
        // Node tests in the half domain: a stored plane a is a half, so a <= y holds exactly when
        // a <= half_down(y), and y <= a exactly when half_up(y) <= a.  The five bounds are rounded
        // once per wave.  A word of the node holds one plane of BOTH children, so the five
        // differences "how far outside" are five packed half subtractions, their maximum four packed
        // max, and a child is met when its half of the result is <= 0 (the difference of two halves is
        // a multiple of 2^-24, so rounding never turns a non-zero difference into zero or flips its
        // sign).  9 vector + 7 scalar instructions per node; written as ten float comparisons the
        // test was a convert, a compare, a select and a readfirstlane each.
        typedef _Float16 half2_t __attribute__((ext_vector_type(2)));
        auto H2 = [](uint32_t w) { return __builtin_bit_cast(half2_t, w); };
        auto both = [](uint32_t h) { return (h & 0xffffu) | (h << 16); };
        const half2_t ydn = H2(both(half_down(yhi))), yup = H2(both(half_up(ylo))), zdn = H2(both(half_down(zhi)));
        const half2_t zup = H2(both(half_up(zlo))), xup = H2(both(half_up(oxMin)));
        auto triangle = [&](const TriPos& tp) {
                if (RB == 1) {
                    const ParityRowTri s = parity_row_setup(oy[0], oz[0], tp.v0, tp.v1, tp.v2);
                    if (s.hit) {
                        uint32_t hits = 0;
#pragma unroll
                        for (int c = 0; c < CH; ++c) hits |= (parity_row_voxel(s, ox[c]) ? 1u : 0u) << c;
                        bits[0] ^= hits;
                    }
                } else {
                    // The per-row set-up is the same arithmetic for every row of the block: lane r does it
                    // for row r (all at once, instead of once per row on wave-uniform values), the rows
                    // that the triangle can cross are then taken one by one, their eight set-up values
                    // broadcast from their lane.
                    const ParityRowTri mine = parity_row_setup(oyLane, ozLane, tp.v0, tp.v1, tp.v2);
                    uint64_t rows = __builtin_amdgcn_ballot_w64(mine.hit) & ((1ull << ROWS) - 1ull);
                    while (rows) {
                        const int r = __builtin_ctzll(rows);
                        rows &= rows - 1ull;
                        auto bc = [r](float v) { return __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), r)); };
                        ParityRowTri s;
                        s.U = bc(mine.U); s.V = bc(mine.V); s.W = bc(mine.W); s.det = bc(mine.det);
                        s.v0x = tp.v0.x; s.v1x = tp.v1.x; s.v2x = tp.v2.x; s.hix = bc(mine.hix); s.hit = true;
                        uint32_t hits = 0;
#pragma unroll
                        for (int c = 0; c < CH; ++c) hits |= (parity_row_voxel(s, ox[c]) ? 1u : 0u) << c;
                        const uint32_t at = (uint32_t)r * CH, word = at >> 5, contrib = hits << (at & 31u);
#pragma unroll
                        for (int w = 0; w < WORDS; ++w) bits[w] ^= word == (uint32_t)w ? contrib : 0u;
                    }
                }
        };
        auto triAt = [&](int32_t leaf) { return load_tri_scalar(sc.triPos, leaf); };
        auto outside = [&](uint32_t xh, uint32_t yl, uint32_t yh, uint32_t zl, uint32_t zh) {   // two children per word; > 0: outside
            half2_t m = __builtin_elementwise_max(__builtin_elementwise_max(H2(yl) - ydn, yup - H2(yh)),
                                                  __builtin_elementwise_max(H2(zl) - zdn, zup - H2(zh)));
            m = __builtin_elementwise_max(m, xup - H2(xh));
            return (uint32_t)__builtin_amdgcn_readfirstlane(__builtin_bit_cast(uint32_t, m));
        };
        if (LISTS) {
            static_assert(!LISTS || RB == 1, "row lists: one row per wave");
            const uint32_t R = sc.plR;
            const uint32_t cell = (uint32_t)__builtin_amdgcn_readfirstlane((int)(dm_texel(oz[0], R) * R + dm_texel(oy[0], R)));
            const uint32_t begin = sc.plCells[2u * cell], count = sc.plCells[2u * cell + 1u];
            const uint32_t* list = sc.plEntries + begin;
            for (uint32_t k = 0; k < count; k += 4u) {
                // four triangle records in flight (the words behind the end of a list are the next list's or the buffer's
                // spare ones: valid slots either way, fetched and not used)
                const uint32_t s0 = list[k], s1 = list[k + 1u], s2 = list[k + 2u], s3 = list[k + 3u];
                const TriPos t0 = load_tri(sc.triPos, (int32_t)s0), t1 = load_tri(sc.triPos, (int32_t)s1);
                const TriPos t2 = load_tri(sc.triPos, (int32_t)s2), t3 = load_tri(sc.triPos, (int32_t)s3);
                triangle(t0);
                if (k + 1u < count) triangle(t1);
                if (k + 2u < count) triangle(t2);
                if (k + 3u < count) triangle(t3);
            }
        } else if (WIDE) {
            walk_parity_rows_wide(
                [&](int32_t i) {
                    const WideSgpr n = load_wide_scalar(sc.wide, i);   // words: x lo, x hi, y lo, y hi, z lo, z hi (children 0,1 | 2,3), links
                    const uint32_t o01 = outside((uint32_t)n.w[1], (uint32_t)n.w[2], (uint32_t)n.w[3], (uint32_t)n.w[4], (uint32_t)n.w[5]);
                    const uint32_t o23 = outside((uint32_t)(n.w[1] >> 32), (uint32_t)(n.w[2] >> 32), (uint32_t)(n.w[3] >> 32),
                                                 (uint32_t)(n.w[4] >> 32), (uint32_t)(n.w[5] >> 32));
                    WideHits r;
                    r.h[0] = (o01 & 0x8000u) != 0u || (o01 & 0x7fffu) == 0u;
                    r.h[1] = (o01 & 0x80000000u) != 0u || (o01 & 0x7fff0000u) == 0u;
                    r.h[2] = (o23 & 0x8000u) != 0u || (o23 & 0x7fffu) == 0u;
                    r.h[3] = (o23 & 0x80000000u) != 0u || (o23 & 0x7fff0000u) == 0u;
                    r.c[0] = (int32_t)(uint32_t)n.w[6]; r.c[1] = (int32_t)(uint32_t)(n.w[6] >> 32);
                    r.c[2] = (int32_t)(uint32_t)n.w[7]; r.c[3] = (int32_t)(uint32_t)(n.w[7] >> 32);
                    return r;
                },
                triAt, stk, triangle);
        } else {
            walk_parity_rows(
                [&](int32_t i) {
                    const NodeSgpr n = load_node_scalar(sc.nodes, i);  // words: x lo, x hi | y lo, y hi | z lo, z hi | links
                    const uint32_t out = outside((uint32_t)(n.w[0] >> 32), (uint32_t)n.w[1], (uint32_t)(n.w[1] >> 32), (uint32_t)n.w[2],
                                                 (uint32_t)(n.w[2] >> 32));
                    NodeHits r;
                    r.h0 = (out & 0x8000u) != 0u || (out & 0x7fffu) == 0u;
                    r.h1 = (out & 0x80000000u) != 0u || (out & 0x7fff0000u) == 0u;
                    r.c0 = (int32_t)(uint32_t)n.w[3];
                    r.c1 = (int32_t)(uint32_t)(n.w[3] >> 32);
                    return r;
                },
                triAt, stk, triangle);
        }
    }
#pragma unroll
    for (int r = 0; r < ROWS; ++r) {
        const size_t rowBase = ((size_t)lz[r / RB] * N + iy[r % RB]) * N;
#pragma unroll
        for (int c = 0; c < CH; ++c) {
            const uint32_t ix = x0 + 64u * c + lane;
            if (ix < N) p.grid[rowBase + ix] = (uint8_t)((bits[(r * CH) / 32] >> ((r * CH) % 32 + c)) & 1u);
        }
    }
#else
    (void)p;
#endif
}

template <int CH, int RB, bool WIDE, bool LISTS = false>
static hipError_t launch_parity_rows_ch(const VoxelizeParams& pin, hipStream_t s)
{
    VoxelizeParams p = pin;
    const uint32_t segLen = 64u * CH, nseg = (p.N + segLen - 1) / segLen;
    const uint64_t nwaves = (uint64_t)((p.N + RB - 1u) / RB) * ((p.nz + RB - 1u) / RB) * nseg;
    uint32_t rb = p.regionBits;
    while (rb > 0 && (8ull << rb) > nwaves) --rb;
    p.regionBits = rb;
    const uint64_t span = 8ull << rb;
    const uint64_t grid = (nwaves + span - 1) / span * span;
    if (grid > 0x7fffffffull) return hipErrorInvalidValue;
    k_parity_rows<CH, RB, WIDE, LISTS><<<dim3((uint32_t)grid), dim3(64), 0, s>>>(p);
    return hipGetLastError();
}

template <int RB, bool WIDE>
static hipError_t launch_parity_rows_rb(const VoxelizeParams& p, hipStream_t s)
{
    if (p.N <= 64) return launch_parity_rows_ch<1, RB, WIDE>(p, s);
    if (p.N <= 128) return launch_parity_rows_ch<2, RB, WIDE>(p, s);
    if (p.N <= 256) return launch_parity_rows_ch<4, RB, WIDE>(p, s);
    return launch_parity_rows_ch<8, RB, WIDE>(p, s);    // 512 voxels per wave; longer rows take several waves
}

// rowBlock: rows per side of a wave's block of rows (1, 2 or 4); the walk takes the four-box nodes when the scene has them
hipError_t launch_parity_rows(const VoxelizeParams& p, int rowBlock, hipStream_t s)
{
    if (p.scene.plCells) {                                             // row lists: one row per wave, no walk
        if (p.N <= 64) return launch_parity_rows_ch<1, 1, false, true>(p, s);
        if (p.N <= 128) return launch_parity_rows_ch<2, 1, false, true>(p, s);
        if (p.N <= 256) return launch_parity_rows_ch<4, 1, false, true>(p, s);
        return launch_parity_rows_ch<8, 1, false, true>(p, s);
    }
    if (p.scene.wide) {
        if (rowBlock == 4) return launch_parity_rows_rb<4, true>(p, s);
        if (rowBlock == 2) return launch_parity_rows_rb<2, true>(p, s);
        return launch_parity_rows_rb<1, true>(p, s);
    }
    if (rowBlock == 4) return launch_parity_rows_rb<4, false>(p, s);
    if (rowBlock == 2) return launch_parity_rows_rb<2, false>(p, s);
    return launch_parity_rows_rb<1, false>(p, s);
}

} // namespace dxv
