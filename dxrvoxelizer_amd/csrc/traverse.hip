// traverse.hip -- the voxelisation kernels: one thread per voxel, one ray per thread.
//
// Replaces DispatchRays(GRID_SIZE, GRID_SIZE*GRID_SIZE, 1) with raygenMain / closestHitMain /
// missMain (Content/Voxelizer.cpp:366-368, Content/Shaders/DXRVoxelizer.hlsl:58-85, :132-148).
//
// Launch shape: a workgroup owns a BX x BY x BZ brick of voxels (default 4x4x4 = one wavefront;
// lanes with neighbouring origins and near-parallel radial rays walk the same nodes).  Bricks are
// numbered along a Morton curve and dealt to the 8 XCDs in runs of 2^regionBits bricks, so each
// private L2 sees compact regions while the uneven per-region cost balances.  Only the bricks the
// exact root early-out cannot clear are launched when that removes a good part of the grid.
// The per-thread traversal stack (shared with the postponed-leaf queue) is an LDS column
// (stack[entry][thread]: consecutive lanes hit consecutive banks); a ray that runs out of it is
// listed and finished by k_voxelize_redo with a deep column, never ignored (dxv_api.hip).
// Parity mode normally runs k_parity_rows (one wave-uniform walk per block of grid rows, parity_rows.hip); the reference rule's
// default path is the work queue (plan_bricks.hip) and the two brick kernels of voxelize_lists.hip.
#include "dxv_brick.h"
#include "dxv_dirmap.h"

namespace dxv {

template <int BX, int BY, int BZ>
struct Brick {
    static constexpr int x = BX, y = BY, z = BZ, threads = BX * BY * BZ;
    static_assert(threads == 64 || threads == 128 || threads == 256, "one voxel per thread, whole wavefronts");
};

// WALK: 0 = leaves tested as met, 1 = postponed-leaf walk, 2 = the same over the wide nodes (MODE 0)
template <class B, int STACK, int MODE, bool TEXELS, int WALK, int ABL = 0>
__global__ __launch_bounds__(B::threads, WALK == 4 ? 6 : 8) void k_voxelize(VoxelizeParams p)   // walks: <= 64 VGPRs, 8 waves/SIMD; lists (WALK 4): 70 VGPRs, 7 waves
{
    __shared__ int32_t stack[STACK * B::threads];
    const uint32_t N = p.N;
    uint32_t bx, by, bz;
    {
    const uint32_t nb = p.nbx * p.nby * p.nbz;
    // XCD-aware remap: workgroups b and b + 8 share an XCD.  Bricks are numbered along a Morton
    // curve (below); runs of 2^regionBits consecutive bricks (compact regions) are dealt round-robin
    // to the 8 XCDs: each XCD's L2 sees compact regions, and the regions of all XCDs are fine
    // grained enough to balance the very uneven per-region cost.
    const uint32_t rb = p.regionBits;
    const uint32_t j = blockIdx.x >> 3;
    const uint32_t lin = ((((j >> rb) << 3) | (blockIdx.x & 7u)) << rb) | (j & ((1u << rb) - 1u));
    if (lin >= nb) return;
    // Consecutive workgroups of an XCD cover a compact region and reuse the same part of the tree in L1/L2.
    brick_of_lin(p, lin, bx, by, bz);
    }
    const uint32_t tid = threadIdx.x;
    const uint32_t ix = bx * B::x + tid % B::x;
    const uint32_t iy = by * B::y + (tid / B::x) % B::y;
    const uint32_t lz = bz * B::z + tid / (B::x * B::y);
    if (ix >= N || iy >= N || lz >= p.nz) return;
    const uint32_t iz = global_slice(p.z0, p.nz, p.zBlock, p.zShift, p.zPeriod, lz);
    const size_t id = ((size_t)lz * N + iy) * N + ix;
    if (MODE == 0 && B::x == 4 && B::y == 4 && B::z == 4 && p.mipR) {
        // The work queue's brick test without a queue (tree walks, plan = 0): can ANY ray of this brick reach a triangle?  p.mip is the
        // max-mip of the far radii of the scene's lists, or -- a scene without lists -- of the triangles' own footprints (dirmap_far).
        // Wave-uniform; a dead brick costs its workgroup a hundred instructions and four loads instead of 64 walks out of the tree.
        float x0, x1, y0, y1, z0, z1;
        dm_brick_hull(N, p.nz, p.z0, p.zBlock, p.zShift, p.zPeriod, bx, by, bz, x0, x1, y0, y1, z0, z1);
        if (!dm_box_may_be_live(x0, x1, y0, y1, z0, z1, p.scene.rootLo, p.scene.rootHi, p.mip, p.mipR)) {
            if (TEXELS) p.texels[id] = 0u;
            p.grid[id] = 0;
            return;
        }
    }

    const StridedStack stk{stack + tid, B::threads};
    bool overflow = false;
    uint8_t occ;
    if (MODE == 0) {
        uint32_t texel = 0;
        occ = voxel_reference<WALK, StridedStack, ABL>(p.scene, N, ix, iy, iz, stk, STACK, TEXELS ? &texel : nullptr, overflow);
        if (TEXELS) p.texels[id] = texel;
    } else {
        occ = voxel_parity<WALK != 0>(p.scene, N, ix, iy, iz, stk, STACK, overflow);
    }
    if (overflow) {
        // this ray needs a deeper column than the launch has: hand the voxel to k_voxelize_redo
        const uint32_t slot = atomicAdd(p.status + 1 + p.redoParity, 1u);
        if (slot < p.redoCap) p.redo[slot] = (uint64_t)id;
        else atomicOr(p.status, 1u);
    }
    p.grid[id] = occ;
}

// The rays whose LDS column was too small in k_voxelize (a few per million: DESIGN.md), one per
// lane with a column of kRedoStack entries -- enough for any tree the builder makes (height <= 62).
// Plain binary walk, leaves tested where they are met; same voxel as every other walk.
constexpr int kRedoStack = 64;
template <int MODE, bool TEXELS>
__global__ __launch_bounds__(64) void k_voxelize_redo(VoxelizeParams p)
{
    __shared__ int32_t stack[kRedoStack * 64];
    const uint32_t mine = 1u + p.redoParity, other = 2u - p.redoParity;
    uint32_t count = p.status[mine];
    if (count > p.redoCap) count = p.redoCap;
    if (blockIdx.x == 0 && threadIdx.x == 0) p.status[other] = 0;      // the next launch appends there
    const StridedStack stk{stack + threadIdx.x, 64};
    const uint64_t plane = (uint64_t)p.N * p.N;
    for (uint32_t i = blockIdx.x * 64u + threadIdx.x; i < count; i += gridDim.x * 64u) {
        const uint64_t id = p.redo[i];
        const uint32_t lz = (uint32_t)(id / plane), rem = (uint32_t)(id % plane), iy = rem / p.N, ix = rem % p.N;
        const uint32_t iz = global_slice(p.z0, p.nz, p.zBlock, p.zShift, p.zPeriod, lz);
        bool overflow = false;
        uint8_t occ;
        if (MODE == 0) {
            uint32_t texel = 0;
            occ = voxel_reference<0>(p.scene, p.N, ix, iy, iz, stk, kRedoStack, TEXELS ? &texel : nullptr, overflow);
            if (TEXELS) p.texels[id] = texel;
        } else occ = voxel_parity<false>(p.scene, p.N, ix, iy, iz, stk, kRedoStack, overflow);
        if (overflow) atomicOr(p.status, 1u);
        p.grid[id] = occ;
    }
}

hipError_t launch_voxelize_redo(const VoxelizeParams& p, hipStream_t s)
{
    const dim3 g(128), b(64);
    if (p.mode == 0) {
        if (p.texels) k_voxelize_redo<0, true><<<g, b, 0, s>>>(p);
        else k_voxelize_redo<0, false><<<g, b, 0, s>>>(p);
    } else k_voxelize_redo<1, false><<<g, b, 0, s>>>(p);
    return hipGetLastError();
}

// brick shapes: (x, y, z) voxels per workgroup; a wavefront owns 64 consecutive threads of it
using Brick0 = Brick<64, 4, 1>;    // 256 threads, wave = 64x1x1 row
using Brick1 = Brick<8, 8, 4>;     // 256 threads, wave = 8x8x1 tile
using Brick2 = Brick<4, 4, 16>;    // 256 threads, wave = 4x4x4 cube
using Brick3 = Brick<16, 4, 4>;    // 256 threads, wave = 16x4x1
using Brick4 = Brick<4, 4, 4>;     // 64 threads,  one wave per workgroup
using Brick5 = Brick<8, 8, 1>;     // 64 threads
using Brick6 = Brick<4, 4, 8>;     // 128 threads
using Brick7 = Brick<8, 4, 2>;     // 64 threads

int num_brick_shapes() { return 8; }

// Voxel index ranges [lo, hi] per axis outside of which origin_leaves_root() is certain (evaluated
// with the very same float formulas on the host).  Returns false when no voxel can be non-zero.
static bool live_ranges(const VoxelizeParams& p, uint32_t lo[3], uint32_t hi[3])
{
    for (int a = 0; a < 3; ++a) {
        const uint32_t n = a == 2 ? p.nz : p.N;
        bool any = false;
        for (uint32_t i = 0; i < n; ++i) {
            float o[3];
            const uint32_t g = a == 2 ? global_slice(p.z0, p.nz, p.zBlock, p.zShift, p.zPeriod, i) : i;
            ray_origin(p.N, a == 0 ? g : 0, a == 1 ? g : 0, a == 2 ? g : 0, o[0], o[1], o[2]);
            if (p.mode == 0 ? axis_leaves_root(o[a], p.scene.rootLo[a], p.scene.rootHi[a])
                            : (a == 0 ? !(p.scene.rootHi[0] >= o[0]) : !(p.scene.rootLo[a] <= o[a] && o[a] <= p.scene.rootHi[a])))
                continue;
            if (!any) lo[a] = i;
            hi[a] = i;
            any = true;
        }
        if (!any) return false;
    }
    return true;
}

template <class B, int STACK>
static hipError_t launch_shape(const VoxelizeParams& pin, hipStream_t s)
{
    VoxelizeParams p = pin;
    const uint32_t tbx = (p.N + B::x - 1) / B::x, tby = (p.N + B::y - 1) / B::y, tbz = (p.nz + B::z - 1) / B::z;
    // launch only the bricks the root early-out cannot clear; everything else is zero by memset
    uint32_t lo[3], hi[3];
    const bool live = live_ranges(p, lo, hi);
    uint32_t b0[3] = {0, 0, 0}, b1[3] = {tbx, tby, tbz};
    if (live && p.subbox) {
        const uint32_t bs[3] = {(uint32_t)B::x, (uint32_t)B::y, (uint32_t)B::z}, tb[3] = {tbx, tby, tbz};
        for (int a = 0; a < 3; ++a) {
            b0[a] = (lo[a] / bs[a]) & ~7u;                       // 8-brick alignment keeps Morton locality
            b1[a] = (hi[a] / bs[a] + 1u + 7u) & ~7u;
            if (b1[a] > tb[a]) b1[a] = tb[a];
        }
    }
    // worth it only when a good part of the grid goes away: the cleared bricks are cheap (their waves
    // fill idle slots) while the memset is serial (measured: -5 % on a thin mesh, +3 % on a full one)
    if (live && (uint64_t)(b1[0] - b0[0]) * (b1[1] - b0[1]) * (b1[2] - b0[2]) * 10u > (uint64_t)tbx * tby * tbz * 6u) {
        b0[0] = b0[1] = b0[2] = 0;
        b1[0] = tbx; b1[1] = tby; b1[2] = tbz;
    }
    const bool partial = !live || b0[0] || b0[1] || b0[2] || b1[0] != tbx || b1[1] != tby || b1[2] != tbz;
    // The memset of a partial launch (the whole grid: 134 MB, 35 us at 512^3) is still good when the frame's last writer was
    // the same partial launch -- same grid, slab, partition, brick box, rule and buffers: the kernel only ever writes inside
    // the box.  The frame's signature word says so; every other writer of the grid resets it (full launches here, the row
    // kernel and reallocations in dxv_api.hip).
    uint64_t sig = 0;
    if (partial && live) {
        auto mix = [&](uint64_t v) { sig = (sig ^ v) * 0x9E3779B97F4A7C15ull; sig ^= sig >> 29; };
        mix(p.N); mix(p.nz); mix(p.z0); mix(p.zBlock); mix(p.zPeriod); mix((uint64_t)p.mode);
        for (int a = 0; a < 3; ++a) { mix(b0[a]); mix(b1[a]); }
        mix((uint64_t)B::x | ((uint64_t)B::y << 16) | ((uint64_t)B::z << 32));
        mix(reinterpret_cast<uint64_t>(p.grid)); mix(reinterpret_cast<uint64_t>(p.texels));
        sig |= 1ull;                                                    // never 0 (= no valid memset)
    }
    if (partial && !(p.clearSig && sig && *p.clearSig == sig)) {
        hipError_t e = hipMemsetAsync(p.grid, 0, (size_t)p.N * p.N * p.nz, s);
        if (e != hipSuccess) return e;
        if (p.texels && (e = hipMemsetAsync(p.texels, 0, (size_t)p.N * p.N * p.nz * 4, s)) != hipSuccess) return e;
    }
    if (p.clearSig) *p.clearSig = sig;                                  // (0 after a full launch or an all-empty grid)
    if (!live) return hipSuccess;
    const uint32_t nbx = b1[0] - b0[0], nby = b1[1] - b0[1], nbz = b1[2] - b0[2];
    p.nbx = nbx; p.nby = nby; p.nbz = nbz;
    p.bx0 = b0[0]; p.by0 = b0[1]; p.bz0 = b0[2];
    uint32_t m = 0;
    while (m < 10 && p.morton && !((nbx >> m) & 1u) && !((nby >> m) & 1u) && !((nbz >> m) & 1u)) ++m;
    p.mortonBits = m;
    p.superX = nbx >> m;
    p.superY = nby >> m;
    const uint64_t nb = (uint64_t)nbx * nby * nbz;
    uint32_t rb = p.regionBits;
    while (rb > 0 && (8ull << rb) > nb) --rb;          // small grids: keep all XCDs busy
    p.regionBits = rb;
    const uint64_t span = 8ull << rb;                  // bricks per round of 8 regions
    const uint64_t grid = (nb + span - 1) / span * span;
    if (grid > 0x7fffffffull) return hipErrorInvalidValue;
    const dim3 g((uint32_t)grid), b(B::threads);
    if (p.mode == 0 && p.lists) {
        // direction-space lists: no stack, the column is the queue of selected triangles (8 entries; 16 for deep scenes,
        // where a ray meets many candidates before its first flush)
        if constexpr (STACK == 8 || STACK == 16) {
#if defined(DXV_ABLATE)                                                  // (only in the library tools/ablate.py builds for itself: libdxv_ablate.so)
            if constexpr (B::threads == 64 && B::x == 4 && STACK == 16) {    // timing-only ablations of the default shape (tools/ablate.py)
                switch (p.ablate) {
                case 0: break;
                case 1: k_voxelize<B, 16, 0, false, 4, 1><<<g, b, 0, s>>>(p); return hipGetLastError();
                case 2: k_voxelize<B, 16, 0, false, 4, 2><<<g, b, 0, s>>>(p); return hipGetLastError();
                case 4: k_voxelize<B, 16, 0, false, 4, 4><<<g, b, 0, s>>>(p); return hipGetLastError();
                case 6: k_voxelize<B, 16, 0, false, 4, 6><<<g, b, 0, s>>>(p); return hipGetLastError();
                case 8: k_voxelize<B, 16, 0, false, 4, 8><<<g, b, 0, s>>>(p); return hipGetLastError();
                case 16: k_voxelize<B, 16, 0, false, 4, 16><<<g, b, 0, s>>>(p); return hipGetLastError();
                case 18: k_voxelize<B, 16, 0, false, 4, 18><<<g, b, 0, s>>>(p); return hipGetLastError();
                case 32: k_voxelize<B, 16, 0, false, 4, 32><<<g, b, 0, s>>>(p); return hipGetLastError();
                case 64: k_voxelize<B, 16, 0, false, 4, 64><<<g, b, 0, s>>>(p); return hipGetLastError();
                default: return hipErrorInvalidValue;
                }
            }
#endif
            if (p.texels) k_voxelize<B, STACK, 0, true, 4><<<g, b, 0, s>>>(p);
            else k_voxelize<B, STACK, 0, false, 4><<<g, b, 0, s>>>(p);
        } else return hipErrorInvalidValue;
    } else if (p.mode == 0) {
        if (p.texels) {
            if (p.wide) k_voxelize<B, STACK, 0, true, 2><<<g, b, 0, s>>>(p);
            else k_voxelize<B, STACK, 0, true, 1><<<g, b, 0, s>>>(p);
        } else if (p.wide == 2) k_voxelize<B, STACK, 0, false, 3><<<g, b, 0, s>>>(p);
        else if (p.wide) k_voxelize<B, STACK, 0, false, 2><<<g, b, 0, s>>>(p);
        else if (p.queued) k_voxelize<B, STACK, 0, false, 1><<<g, b, 0, s>>>(p);
        else k_voxelize<B, STACK, 0, false, 0><<<g, b, 0, s>>>(p);
    } else {
        if (p.queued) k_voxelize<B, STACK, 1, false, 1><<<g, b, 0, s>>>(p);
        else k_voxelize<B, STACK, 1, false, 0><<<g, b, 0, s>>>(p);
    }
    return hipGetLastError();
}

int stack_round_up(int want);
// Column depths a brick shape is compiled for: all eight for the shipped shape (4 x 4 x 4: the adaptive column and its
// tuning), three for the shapes that exist for sweeps and cross-checks (16: the lists' queue, 20: the walks' default,
// 64: always sufficient).  A depth in between takes the next one up -- a deeper column than asked is never wrong.
int stack_for_brick(int brickShape, int want)
{
    want = stack_round_up(want);
    if (brickShape == 4) return want;
    return want <= 16 ? 16 : want <= 20 ? 20 : 64;
}

template <class B>
static hipError_t launch_stack(const VoxelizeParams& p, int stackEntries, hipStream_t s)
{
    if constexpr (B::x == 4 && B::y == 4 && B::z == 4) {
        switch (stackEntries) {
        case 8: return launch_shape<B, 8>(p, s);
        case 12: return launch_shape<B, 12>(p, s);
        case 16: return launch_shape<B, 16>(p, s);
        case 20: return launch_shape<B, 20>(p, s);
        case 24: return launch_shape<B, 24>(p, s);
        case 32: return launch_shape<B, 32>(p, s);
        case 48: return launch_shape<B, 48>(p, s);
        default: return launch_shape<B, 64>(p, s);
        }
    } else {
        switch (stackEntries) {
        case 16: return launch_shape<B, 16>(p, s);
        case 20: return launch_shape<B, 20>(p, s);
        case 64: return launch_shape<B, 64>(p, s);
        default: return hipErrorInvalidValue;              // (stack_for_brick maps every depth to one of the three)
        }
    }
}

// The stack holds internal nodes only, one entry per level at most: treeHeight entries always
// suffice.  Smallest instantiated depth >= want (LDS = depth * 4 B per thread).
int stack_round_up(int want)
{
    const int sizes[] = {8, 12, 16, 20, 24, 32, 48, 64};
    for (int v : sizes) if (want <= v) return v;
    return 64;
}

hipError_t launch_voxelize(const VoxelizeParams& p, int brickShape, int stackEntries, hipStream_t s)
{
    if (stack_round_up(stackEntries) != stackEntries || stack_for_brick(brickShape, stackEntries) != stackEntries) return hipErrorInvalidValue;
    switch (brickShape) {
    case 0: return launch_stack<Brick0>(p, stackEntries, s);
    case 1: return launch_stack<Brick1>(p, stackEntries, s);
    case 2: return launch_stack<Brick2>(p, stackEntries, s);
    case 3: return launch_stack<Brick3>(p, stackEntries, s);
    case 4: return launch_stack<Brick4>(p, stackEntries, s);
    case 5: return launch_stack<Brick5>(p, stackEntries, s);
    case 6: return launch_stack<Brick6>(p, stackEntries, s);
    case 7: return launch_stack<Brick7>(p, stackEntries, s);
    default: return hipErrorInvalidValue;
    }
}

} // namespace dxv
