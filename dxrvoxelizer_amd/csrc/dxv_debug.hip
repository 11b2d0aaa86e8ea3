// dxv_debug.hip -- test hooks of the C-ABI: the exhaustive device checks of the lists' superset claim, of the triangle classes
// and of the work queue -- each checker kernel in front of the one entry that calls it --, the grid operators' scan on the caller's numbers
// and the download of internal arrays.
// Not product paths.
#include "dxv_ctx.h"
#include "dxv_brick.h"

using namespace dxv;
using namespace dxvhost;

#if defined(DXV_PHASE_TIMES)
namespace dxv { hipError_t phase_times_read(unsigned long long out[16], bool reset); }     // voxelize_lists.hip (its copy of the counters: the two brick kernels'), diagnostic build only
#endif

namespace dxv {
// ---------------------------------------------------------------------------------------------
// Test hook (dxv_debug_list_check): the lists' superset claim, checked exhaustively on the device.  For every voxel the
// LBVH is walked WITHOUT distance culling; every triangle the canonical step accepts for the ray (own padded box passed,
// watertight hit at 0 < t < TMax, box entry <= t) must be found in the ray's texel list and pass that entry's integer
// test (box, edge, radial range) even with the radial cut already drawn at its own t, and lie in front of the point where a
// scan holding a hit at that t stops -- then no order of scanning, no
// cut by an earlier hit and no early stop can keep the closest hit out of the queue (dxv_dirmap.h).  The entry must also lie at or
// behind the start the lists' start table gives this ray (dm_start_offset; the table as it stands in memory, whatever option
// starttable says): a wrong or stale table shows up as violations.
// out[0] accepted (ray, triangle) pairs, out[1] violations, out[2 + 2 k], out[3 + 2 k]: voxel id and triangle slot of the
// first 16 violations.  Not a product path.
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(64) void k_list_check(VoxelizeParams p, unsigned long long* out)
{
    __shared__ int32_t stack[64 * 64];
    const uint32_t N = p.N, nbx = (N + 3u) / 4u;
    const uint32_t b = blockIdx.x, bx = b % nbx, by = (b / nbx) % nbx, bz = b / (nbx * nbx);
    const uint32_t lane = threadIdx.x;
    uint32_t ix, iy, lz;
    brick_voxel(bx, by, bz, lane, ix, iy, lz);
    const uint32_t iz = p.z0 + lz;
    if (ix >= N || iy >= N || lz >= p.nz) return;
    const SceneView& sc = p.scene;
    Ray r;
    ray_origin(N, ix, iy, iz, r.ox, r.oy, r.oz);
    if (origin_leaves_root(r.ox, r.oy, r.oz, sc.rootLo, sc.rootHi)) return;
    finish_ray_reference(r);
    ray_shear(r);
    const DirMapView dm{static_cast<const DirCell*>(sc.dmCells), static_cast<const DirEntry*>(sc.dmEntries), sc.dmR, 0u, sc.dmStarts};
    const DirRayStart start = dm_ray_start(r.ox, r.oy, r.oz, dm);
    const DirCell cell = start.cell;
    const DirRayLocal loc = dm_ray_local(start.cx, start.cy);
    const float rho = start.rho, near = start.near;
    const uint32_t from = cell.begin + dm_start_offset(start.startWord, cell.count, cell.r1max, near);
    const size_t id = ((size_t)lz * N + iy) * N + ix;
    auto leaf = [&](int32_t l) {
        const TriPos tp = load_tri(sc.triPos, l);
        float lo[3], hi[3], tn, t, b1, b2;
        tri_box(tp.v0, tp.v1, tp.v2, lo, hi);
        if (!slab(r, lo[0], lo[1], lo[2], hi[0], hi[1], hi[2], tn)) return;
        if (!tri_test<false>(r, tp.v0, tp.v1, tp.v2, t, b1, b2) || tn > t) return;
        atomicAdd(out, 1ull);
        const uint32_t rc = dm_radial_word(near, (rho + t) * 1.001f + 1e-4f);
        bool found = false;
        const float step = dm_stop_step(half_bits_to_float(cell.thick)), bound = (rho + t) * 1.001f + 1e-4f;
        if (start.live)
            for (uint32_t k = from; k < cell.begin + cell.count && !found; ++k) {
                const DirEntry e = dm.entries[k];
                if (dm_stop_radius(e, step) > bound) break;             // a scan with this hit in hand would stop here: the entry must come before
                found = dm_entry_tri(e) == (uint32_t)l && dm_local_pass(e, loc, rc);
            }
        if (!found) {
            const unsigned long long slot = atomicAdd(out + 1, 1ull);
            if (slot < 16ull) { out[2 + 2 * slot] = (unsigned long long)id; out[3 + 2 * slot] = (unsigned long long)(uint32_t)l; }
        }
    };
    int32_t* stk = stack + lane;
    int sp = 0;
    int32_t node = 0;
    for (;;) {
        const NodePlanes n = load_node(sc.nodes, node);
        float tn0, tn1;
        const bool h0 = slab(r, n.b[0], n.b[1], n.b[2], n.b[3], n.b[4], n.b[5], tn0);
        const bool h1 = slab(r, n.b[6], n.b[7], n.b[8], n.b[9], n.b[10], n.b[11], tn1);
        if (h0 && n.c0 < 0) leaf(~n.c0);
        if (h1 && n.c1 < 0) leaf(~n.c1);
        const bool i0 = h0 && n.c0 >= 0, i1 = h1 && n.c1 >= 0;
        if (i0 && i1) { if (sp < 64) stk[64 * sp++] = n.c1; node = n.c0; }
        else if (i0) node = n.c0;
        else if (i1) node = n.c1;
        else {
            if (sp == 0) break;
            node = stk[64 * --sp];
        }
    }
}

static hipError_t launch_list_check(const VoxelizeParams& p, unsigned long long* out, hipStream_t s)
{
    const uint32_t nb = (p.N + 3u) / 4u, nbz = (p.nz + 3u) / 4u;
    k_list_check<<<dim3(nb * nb * nbz), dim3(64), 0, s>>>(p, out);
    return hipGetLastError();
}
} // namespace dxv

// one checker over `words` zeroed 64-bit counters on stream s, the first `back` of them read into out
template <class LaunchFn>
static int run_check(dxv_ctx* c, const char* who, size_t words, size_t back, uint64_t* out, hipStream_t s, LaunchFn launch)
{
    DevBuf<unsigned long long> d;                                       // (a temporary of the call: freed when it returns)
    DXV_HIP(c, d.reserve(words, words * sizeof(unsigned long long)));
    hipError_t e = hipMemsetAsync(d.p, 0, words * sizeof(unsigned long long), s);
    if (e == hipSuccess) e = launch(d.p);
    if (e == hipSuccess) e = hipMemcpyAsync(out, d.p, back * sizeof(unsigned long long), hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    if (e != hipSuccess) return fail(c, "%s failed: %s", who, hipGetErrorString(e));
    return 0;
}

extern "C" int dxv_debug_list_check(dxv_ctx* c, uint32_t N, uint32_t z0, uint32_t nz, uint64_t out[34])
{
    if (!c || !out) return 1;
    if (!c->haveScene) return fail(c, "dxv_debug_list_check: no scene");
    if (check_slab(c, "dxv_debug_list_check", N, z0, nz)) return 1;
    if (c->hdr.treeHeight + 1 > 64) return fail(c, "dxv_debug_list_check: tree too deep for the checker's stack");
    DXV_HIP(c, hipSetDevice(c->device));
    if (sync_frames(c)) return 1;
    if (c->lists.state == 0 || c->lists.opt != c->opt.listres) {
        if (build_lists(c, c->stream)) return 1;
    }
    if (c->lists.state != 1) return fail(c, "dxv_debug_list_check: this scene has no lists (over the caps)");
    if (ensure_nodes(c, c->stream)) return 1;
    VoxelizeParams p{};
    scene_params(c, p.scene);
    lists_params(c, p.scene);
    p.scene.dmStarts = c->lists.starts.p;
    p.N = N; p.z0 = z0; p.nz = nz;
    return run_check(c, "dxv_debug_list_check", 34, 34, out, c->stream, [&](unsigned long long* d) { return launch_list_check(p, d, c->stream); });
}

namespace dxv {
// ---------------------------------------------------------------------------------------------
// Test hook (dxv_debug_class_check): the per-triangle class of the normal test (normal_class, dxv_math.h: "every ray of the
// rule that can hit this triangle gets the same answer from the predicate"), checked against the predicate itself for
// every closest hit of a grid.  The closest hit comes from the plain LBVH walk (no lists, no shortcut); when its triangle
// carries a class, the canonical predicate (hlsl:137-138: interpolated normal, normalize, dot > 0.12) is evaluated as for
// an unclassified triangle and must agree.  out[0] hits on classified triangles, out[1] disagreements, out[2] all hits,
// out[3 + 2 k], out[4 + 2 k]: voxel id and triangle slot of the first 15 disagreements.  Not a product path.
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(64) void k_class_check(VoxelizeParams p, unsigned long long* out)
{
    __shared__ int32_t stack[64 * 64];
    const uint32_t N = p.N, nbx = (N + 3u) / 4u;
    const uint32_t b = blockIdx.x, bx = b % nbx, by = (b / nbx) % nbx, bz = b / (nbx * nbx);
    const uint32_t lane = threadIdx.x;
    uint32_t ix, iy, lz;
    brick_voxel(bx, by, bz, lane, ix, iy, lz);
    const uint32_t iz = p.z0 + lz;
    if (ix >= N || iy >= N || lz >= p.nz) return;
    const SceneView& sc = p.scene;
    Ray r;
    ray_origin(N, ix, iy, iz, r.ox, r.oy, r.oz);
    if (origin_leaves_root(r.ox, r.oy, r.oz, sc.rootLo, sc.rootHi)) return;
    finish_ray_reference(r);
    const StridedStack stk{stack + lane, 64};
    Hit best;
    if (!trace_reference(r, sc.nodes, sc.triPos, stk, 64, best)) { atomicAdd(out + 1, 1ull); return; }     // (cannot happen: 64 >= any tree height)
    if (best.k == 0xffffffffu) return;
    atomicAdd(out + 2, 1ull);
    const TriPos tp = load_tri(sc.triPos, best.leaf);
    const uint32_t cls = __builtin_bit_cast(uint32_t, tp.v1.w) >> kClassShift;
    if (cls == 0u) return;
    atomicAdd(out, 1ull);
    const TriNrm tn = sc.triNrm[best.leaf];
    float nx, ny, nz;
    const bool in = predicate(r, tn.n0, tn.n1, tn.n2, best.b1, best.b2, nx, ny, nz);
    if (in != (cls == kClassIn)) {
        const unsigned long long slot = atomicAdd(out + 1, 1ull);
        if (slot < 15ull) { out[3 + 2 * slot] = ((unsigned long long)lz * N + iy) * N + ix; out[4 + 2 * slot] = (unsigned long long)(uint32_t)best.leaf; }
    }
}

static hipError_t launch_class_check(const VoxelizeParams& p, unsigned long long* out, hipStream_t s)
{
    const uint32_t nb = (p.N + 3u) / 4u, nbz = (p.nz + 3u) / 4u;
    k_class_check<<<dim3(nb * nb * nbz), dim3(64), 0, s>>>(p, out);
    return hipGetLastError();
}
} // namespace dxv

extern "C" int dxv_debug_class_check(dxv_ctx* c, uint32_t N, uint32_t z0, uint32_t nz, uint64_t out[34])
{
    if (!c || !out) return 1;
    if (!c->haveScene) return fail(c, "dxv_debug_class_check: no scene");
    if (check_slab(c, "dxv_debug_class_check", N, z0, nz)) return 1;
    if (c->hdr.treeHeight + 1 > 64) return fail(c, "dxv_debug_class_check: tree too deep for the checker's stack");
    DXV_HIP(c, hipSetDevice(c->device));
    if (sync_frames(c)) return 1;
    if (ensure_nodes(c, c->stream)) return 1;
    VoxelizeParams p{};
    scene_params(c, p.scene);
    p.N = N; p.z0 = z0; p.nz = nz;
    return run_check(c, "dxv_debug_class_check", 34, 34, out, c->stream, [&](unsigned long long* d) { return launch_class_check(p, d, c->stream); });
}

namespace dxv {
// ---------------------------------------------------------------------------------------------
// Test hook (dxv_debug_division_check): the ray set-up's scale-free divisions (dxv_math.h: rcp_refined / div_by) against the IEEE
// quotient `/` the host computes, for EVERY voxel origin of an N^3 grid: origin (grids whose side is no power of two divide by N), the
// cube-map point (u, v) and start radius, direction, 1 / direction, the three shear constants -- 15 words per voxel, compared bit for bit.
// out[0] voxels, out[1] voxels with a differing word (must be 0), out[2 + k]: id of the first 6.  Not a product path.
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_division_check(uint32_t N, unsigned long long* out)
{
    const uint32_t ix = blockIdx.x * 256u + threadIdx.x, iy = blockIdx.y, iz = blockIdx.z;      // (one grid row per (y, z): no 64-bit index arithmetic)
    if (ix >= N) return;
    const uint64_t id = ((uint64_t)iz * N + iy) * N + ix;
    // the product's own code
    Ray r;
    ray_origin(N, ix, iy, iz, r.ox, r.oy, r.oz);
    uint32_t face;
    float u, v, rho;
    dm_ray_point(r.ox, r.oy, r.oz, face, u, v, rho);
    finish_ray_reference(r, rho);
    ray_shear_finished(r);
    // the same with IEEE quotients
    const float fn = (float)N;
    float ox, oy, oz;
    if ((N & (N - 1u)) == 0u) { ox = r.ox; oy = r.oy; oz = r.oz; }      // (a power of two multiplies by an exact reciprocal: no division there)
    else {
        ox = ((float)ix + 0.5f) / fn * 2.0f - 1.0f;
        oy = -(((float)iy + 0.5f) / fn * 2.0f - 1.0f);
        oz = ((float)iz + 0.5f) / fn * 2.0f - 1.0f;
    }
    const float ax = __builtin_fabsf(ox), ay = __builtin_fabsf(oy), az = __builtin_fabsf(oz);
    float wu, wv;
    if (ax >= ay && ax >= az) { wu = oy / ax; wv = oz / ax; }
    else if (ay >= az) { wu = oz / ay; wv = ox / ay; }
    else { wu = ox / az; wv = oy / az; }
    const float len = __builtin_sqrtf((ox * ox + oy * oy) + oz * oz);
    const float dx = ox / len, dy = oy / len, dz = oz / len;
    const float ivx = 1.0f / dx, ivy = 1.0f / dy, ivz = 1.0f / dz;
    int kz = 0;
    float m = abs_(dx);
    if (abs_(dy) > m) { kz = 1; m = abs_(dy); }
    if (abs_(dz) > m) { kz = 2; }
    int kx = kz == 2 ? 0 : kz + 1, ky = kx == 2 ? 0 : kx + 1;
    const float dkz = sel3(dx, dy, dz, kz);
    if (dkz < 0.0f) { const int t = kx; kx = ky; ky = t; }
    const float Sx = sel3(dx, dy, dz, kx) / dkz, Sy = sel3(dx, dy, dz, ky) / dkz, Sz = 1.0f / dkz;
    auto ne = [](float a, float b) { return __builtin_bit_cast(uint32_t, a) != __builtin_bit_cast(uint32_t, b); };
    const bool bad = ne(ox, r.ox) || ne(oy, r.oy) || ne(oz, r.oz) || ne(wu, u) || ne(wv, v) || ne(len, rho) || ne(dx, r.dx) || ne(dy, r.dy) || ne(dz, r.dz) ||
                     ne(ivx, r.ivx) || ne(ivy, r.ivy) || ne(ivz, r.ivz) || ne(Sx, r.Sx) || ne(Sy, r.Sy) || ne(Sz, r.Sz) || kz != r.kz;
    // (the count of voxels: one add per grid SLICE -- an add per wave on one word was 90 % of this kernel's time)
    if (blockIdx.x == 0u && blockIdx.y == 0u && threadIdx.x == 0u) atomicAdd(out, (unsigned long long)N * N);
    const unsigned long long mb = __ballot(bad);
    if (mb && (threadIdx.x & 63u) == (uint32_t)__builtin_ctzll(mb)) atomicAdd(out + 1, (unsigned long long)__builtin_popcountll(mb));
    if (bad) {
        const unsigned long long slot = atomicAdd(out + 8, 1ull);
        if (slot < 6ull) out[2 + slot] = id;
    }
}
static hipError_t launch_division_check(uint32_t N, unsigned long long* out, hipStream_t s)
{
    k_division_check<<<dim3((N + 255u) / 256u, N, N), dim3(256), 0, s>>>(N, out);
    return hipGetLastError();
}
} // namespace dxv

extern "C" int dxv_debug_division_check(dxv_ctx* c, uint32_t n_first, uint32_t n_last, uint64_t out[8])
{
    if (!c || !out) return 1;
    if (n_first < 2 || (n_first & 1u) || n_last > 2048 || n_last < n_first) return fail(c, "dxv_debug_division_check: need even 2 <= n_first <= n_last <= 2048");
    DXV_HIP(c, hipSetDevice(c->device));
    return run_check(c, "dxv_debug_division_check", 10, 8, out, c->stream, [&](unsigned long long* d) {
        hipError_t e = hipSuccess;
        for (uint32_t N = n_first; N <= n_last && e == hipSuccess; N += 2u) e = launch_division_check(N, d, c->stream);
        return e;
    });
}

namespace dxv {
// ---------------------------------------------------------------------------------------------
// Test hook (dxv_debug_far_check): the brick test of the launches over the brick box -- "no ray of a brick the test calls dead hits
// anything" -- checked exhaustively: for every brick of slices [p.z0, p.z0 + p.nz) the test k_voxelize makes (dm_box_may_be_live
// against p.mip), and for every voxel of a brick it calls dead the plain LBVH walk without any shortcut but the provable root
// early-out.  out[0] bricks, out[1] bricks called dead, out[2] their rays walked, out[3] rays among them with a hit (must be 0),
// out[4 + k]: voxel id of the first 8.  Not a product path.
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(64) void k_far_check(VoxelizeParams p, unsigned long long* out)
{
    __shared__ int32_t stack[64 * 64];
    const uint32_t N = p.N, nbx = (N + 3u) / 4u;
    const uint32_t b = blockIdx.x, bx = b % nbx, by = (b / nbx) % nbx, bz = b / (nbx * nbx);
    const uint32_t lane = threadIdx.x;
    float x0, x1, y0, y1, z0, z1;
    dm_brick_hull(N, p.nz, p.z0, p.nz, 0u, p.nz, bx, by, bz, x0, x1, y0, y1, z0, z1);
    const bool live = dm_box_may_be_live(x0, x1, y0, y1, z0, z1, p.scene.rootLo, p.scene.rootHi, p.mip, p.mipR);
    if (lane == 0u) { atomicAdd(out, 1ull); if (!live) atomicAdd(out + 1, 1ull); }
    if (live) return;
    uint32_t ix, iy, lz;
    brick_voxel(bx, by, bz, lane, ix, iy, lz);
    const uint32_t iz = p.z0 + lz;
    if (ix >= N || iy >= N || lz >= p.nz) return;
    const SceneView& sc = p.scene;
    Ray r;
    ray_origin(N, ix, iy, iz, r.ox, r.oy, r.oz);
    if (origin_leaves_root(r.ox, r.oy, r.oz, sc.rootLo, sc.rootHi)) return;
    finish_ray_reference(r);
    atomicAdd(out + 2, 1ull);
    const StridedStack stk{stack + lane, 64};
    Hit best;
    const bool done = trace_reference(r, sc.nodes, sc.triPos, stk, 64, best);
    if (!done || best.k != 0xffffffffu) {
        const unsigned long long slot = atomicAdd(out + 3, 1ull);
        if (slot < 8ull) out[4 + slot] = ((unsigned long long)lz * N + iy) * N + ix;
    }
}
static hipError_t launch_far_check(const VoxelizeParams& p, unsigned long long* out, hipStream_t s)
{
    const uint32_t nb = (p.N + 3u) / 4u, nbz = (p.nz + 3u) / 4u;
    k_far_check<<<dim3(nb * nb * nbz), dim3(64), 0, s>>>(p, out);
    return hipGetLastError();
}
} // namespace dxv

extern "C" int dxv_debug_far_check(dxv_ctx* c, uint32_t N, uint32_t z0, uint32_t nz, int lists_mip, uint64_t out[12])
{
    if (!c || !out) return 1;
    if (!c->haveScene) return fail(c, "dxv_debug_far_check: no scene");
    if (check_slab(c, "dxv_debug_far_check", N, z0, nz)) return 1;
    if (c->hdr.treeHeight + 1 > 64) return fail(c, "dxv_debug_far_check: tree too deep for the checker's stack");
    DXV_HIP(c, hipSetDevice(c->device));
    if (sync_frames(c)) return 1;
    if (ensure_nodes(c, c->stream)) return 1;
    VoxelizeParams p{};
    scene_params(c, p.scene);
    p.N = N; p.z0 = z0; p.nz = nz;
    if (lists_mip) {
        if (c->lists.state != 1 || !c->lists.mip.p) return fail(c, "dxv_debug_far_check: this scene has no lists");
        p.mip = c->lists.mip.p; p.mipR = c->lists.res;
    } else {
        if (ensure_far_map(c, c->stream)) return 1;
        p.mip = c->farMap.mip.p; p.mipR = c->farMap.R;
    }
    return run_check(c, "dxv_debug_far_check", 12, 12, out, c->stream, [&](unsigned long long* d) { return launch_far_check(p, d, c->stream); });
}

namespace dxv {
// ---------------------------------------------------------------------------------------------
// Test hook (dxv_debug_plan_check): the queue's claim -- no live ray sits in a brick that is not queued -- checked
// exhaustively.  k_plan_mark sets one bit per queued brick (and counts bricks queued twice); k_plan_check makes, for every
// voxel of the partition, exactly the decision the kernel's first step makes (origin_leaves_root, dm_ray_start: the same
// functions) and requires the brick of every live voxel to be marked.
// out[0] live voxels, out[1] bricks with a live voxel, out[2] queued bricks, out[3] violations (must be 0), out[4] bricks
// queued more than once (must be 0), out[5 + k]: brick word of the first 11 violations.  Not a product path.
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_plan_mark(VoxelizeParams p, uint32_t* __restrict__ bits, unsigned long long* __restrict__ out)
{
    const uint32_t nbx = (p.N + 3u) / 4u;
    for (uint32_t x = 0; x < 8u; ++x) {
        const uint32_t heavy = p.queue[queue_heavy_word(x)], len = heavy + p.queue[queue_len_word(x)];
        for (uint32_t k = blockIdx.x * 256u + threadIdx.x; k < len; k += gridDim.x * 256u) {
            const uint32_t w = p.queueSlots[(size_t)x * p.queueCap + queue_slot(k, heavy, p.queueCap)];
            const uint32_t id = ((w >> 20) * nbx + ((w >> 10) & 1023u)) * nbx + (w & 1023u);
            const uint32_t old = atomicOr(bits + (id >> 5), 1u << (id & 31u));
            if (old & (1u << (id & 31u))) atomicAdd(out + 4, 1ull);
            atomicAdd(out + 2, 1ull);
        }
    }
}
__global__ __launch_bounds__(64) void k_plan_check(VoxelizeParams p, uint32_t nb, const uint32_t* __restrict__ bits, unsigned long long* __restrict__ out)
{
    const uint32_t lin = blockIdx.x;
    if (lin >= nb) return;
    uint32_t bx, by, bz;
    brick_of_lin(p, lin, bx, by, bz);
    const uint32_t tid = threadIdx.x, N = p.N;
    uint32_t ix, iy, lz;
    brick_voxel(bx, by, bz, tid, ix, iy, lz);
    bool live = false;
    if (ix < N && iy < N && lz < p.nz) {
        const uint32_t iz = global_slice(p.z0, p.nz, p.zBlock, p.zShift, p.zPeriod, lz);
        float ox, oy, oz;
        ray_origin(N, ix, iy, iz, ox, oy, oz);
        if (!origin_leaves_root(ox, oy, oz, p.scene.rootLo, p.scene.rootHi)) {
            const DirMapView dm{static_cast<const DirCell*>(p.scene.dmCells), static_cast<const DirEntry*>(p.scene.dmEntries), p.scene.dmR};
            live = dm_ray_start(ox, oy, oz, dm).live;
        }
    }
    const unsigned long long m = __ballot(live);
    if (tid != 0u || !m) return;
    atomicAdd(out, (unsigned long long)__builtin_popcountll(m));
    atomicAdd(out + 1, 1ull);
    const uint32_t nbx = (N + 3u) / 4u, id = (bz * nbx + by) * nbx + bx;
    if (!(bits[id >> 5] & (1u << (id & 31u)))) {
        const unsigned long long slot = atomicAdd(out + 3, 1ull);
        if (slot < 11ull) out[5 + slot] = bx | (by << 10) | (bz << 20);
    }
}
static hipError_t launch_plan_check(const VoxelizeParams& pin, uint32_t* bits, unsigned long long* out, hipStream_t s)
{
    VoxelizeParams p = pin;
    const uint32_t nb = plan_layout(p);
    hipError_t e = hipMemsetAsync(bits, 0, sizeof(uint32_t) * (((size_t)nb + 31u) / 32u), s);
    if (e == hipSuccess) e = hipMemsetAsync(out, 0, 16 * sizeof(unsigned long long), s);
    if (e != hipSuccess) return e;
    k_plan_mark<<<dim3(256), dim3(256), 0, s>>>(p, bits, out);
    k_plan_check<<<dim3(nb), dim3(64), 0, s>>>(p, nb, bits, out);
    return hipGetLastError();
}
} // namespace dxv

extern "C" int dxv_debug_plan_check(dxv_ctx* c, uint64_t out[16])
{
    if (!c || !out) return 1;
    Frame& f = cur_frame(c);
    if (settle_lists(c)) return 1;
    // (the frame's last launch ran a queue of the context's: still the one for that partition?  A slot may have been reused since)
    bool prepared = f.lastPrepared >= 0 && c->prepared[f.lastPrepared].epoch == c->listEpoch;
    if (prepared) {
        const auto& q = c->prepared[f.lastPrepared];
        prepared = q.N == f.grid_dim && q.z0 == f.z0 && q.nz == f.nz && q.zBlock == f.lastZBlock && q.zPeriod == f.lastZPeriod && q.mem.p;
    }
    if (!c->haveScene || c->lists.state != 1 || !(prepared || (f.lastQueued && f.queue.p)) || !f.grid_dim)
        return fail(c, "dxv_debug_plan_check: the current frame's last launch did not go through a work queue");
    DXV_HIP(c, hipSetDevice(c->device));
    if (sync_frames(c)) return 1;
    const hipStream_t fs = cur_stream(c);
    VoxelizeParams p{};
    scene_params(c, p.scene);
    lists_params(c, p.scene);
    p.N = f.grid_dim; p.z0 = f.z0; p.nz = f.nz; p.zBlock = f.lastZBlock; p.zPeriod = f.lastZPeriod; p.zShift = z_shift(p.zBlock);
    uint32_t cap = 0;
    (void)plan_queue_words(p.N, p.nz, &cap);
    p.queue = f.queue.p + f.queueHdr * kQueueHeaderWords; p.queueSlots = f.queue.p + kQueueSlotsAt; p.queueCap = cap; p.mip = c->lists.mip.p;
    if (prepared) {                                                     // (a queue of the context's, built by dxv_prepare_launch: same layout behind ONE header)
        const auto& q = c->prepared[f.lastPrepared];
        p.queue = q.mem.p; p.queueSlots = q.mem.p + kQueueHeaderWords; p.queueCap = q.cap;
    }
    VoxelizeParams q = p;
    const uint32_t nb = plan_layout(q);
    DevBuf<uint32_t> bits;
    DevBuf<unsigned long long> dOut;
    DXV_HIP(c, bits.reserve(((size_t)nb + 31u) / 32u, sizeof(uint32_t) * (((size_t)nb + 31u) / 32u)));
    hipError_t e = dOut.reserve(16, 16 * sizeof(unsigned long long));
    if (e == hipSuccess) e = launch_plan_check(p, bits.p, dOut.p, fs);
    if (e == hipSuccess) e = hipMemcpyAsync(out, dOut.p, 16 * sizeof(unsigned long long), hipMemcpyDeviceToHost, fs);
    if (e == hipSuccess) e = hipStreamSynchronize(fs);
    if (e != hipSuccess) return fail(c, "dxv_debug_plan_check failed: %s", hipGetErrorString(e));
    return 0;
}

// the order of the PREPARED queue the current frame's last launch ran (queue_order.hip: k_order_check)
extern "C" int dxv_debug_queue_order(dxv_ctx* c, uint64_t out[4])
{
    if (!c || !out) return 1;
    Frame& f = cur_frame(c);
    if (settle_lists(c)) return 1;
    const int slot = f.lastPrepared;
    if (!c->haveScene || c->lists.state != 1 || slot < 0 || c->prepared[slot].epoch != c->listEpoch || !c->prepared[slot].mem.p)
        return fail(c, "dxv_debug_queue_order: the current frame's last launch did not go through a prepared queue");
    const auto& q = c->prepared[slot];
    DXV_HIP(c, hipSetDevice(c->device));
    if (sync_frames(c)) return 1;
    const hipStream_t fs = cur_stream(c);
    VoxelizeParams p{};
    scene_params(c, p.scene);
    lists_params(c, p.scene);
    p.N = q.N; p.z0 = q.z0; p.nz = q.nz; p.zBlock = q.zBlock; p.zPeriod = q.zPeriod; p.zShift = z_shift(q.zBlock);
    p.queue = q.mem.p; p.queueSlots = q.mem.p + kQueueHeaderWords; p.queueCap = q.cap;
    DevBuf<uint32_t> tiles;
    DevBuf<unsigned long long> dOut;
    DXV_HIP(c, tiles.reserve(queue_order_check_words(), sizeof(uint32_t) * queue_order_check_words()));
    hipError_t e = dOut.reserve(4, 4 * sizeof(unsigned long long));
    if (e == hipSuccess) e = launch_queue_order_check(p, tiles.p, dOut.p, fs);
    if (e == hipSuccess) e = hipMemcpyAsync(out, dOut.p, 4 * sizeof(unsigned long long), hipMemcpyDeviceToHost, fs);
    if (e == hipSuccess) e = hipStreamSynchronize(fs);
    if (e != hipSuccess) return fail(c, "dxv_debug_queue_order failed: %s", hipGetErrorString(e));
    return 0;
}

// scan.hip's two entry points on the caller's numbers, in place: up, one launch_scan_*, down.  What the launchers refuse -- a lane count that is
// neither 1 nor 2, nothing to scan, no buffer (host == NULL is handed on as it is) -- comes back as their error, and `host` is not written.
// The hook itself admits up to 4 lanes, so that a lane count of 3 reaches the launchers and is refused THERE.
extern "C" int dxv_debug_scan(dxv_ctx* c, int what, uint32_t lanes, void* host, size_t items, uint64_t totals[2])
{
    if (!c || !totals) return 1;
    if (what != 0 && what != 1) return fail(c, "dxv_debug_scan: unknown selector %d", what);
    if (lanes > 4u || items > (size_t(1) << 26)) return fail(c, "dxv_debug_scan: at most 4 lanes and 2^26 items");      // (a test hook's allocations stay small)
    DXV_HIP(c, hipSetDevice(c->device));
    const hipStream_t s = c->stream;
    const size_t n = items * lanes, blocks = what == 0 ? scan_blocks(items) : 0;      // (block sums: the scratch of launch_scan_words alone)
    const size_t bytes = what == 0 ? n * sizeof(uint32_t) : (n + lanes + 1u) * sizeof(unsigned long long);    // what = 1: sums, totals, a guard word
    DevBuf<uint8_t> d;
    DevBuf<unsigned long long> work;                                    // what = 0: the block sums, then the totals
    if (host) DXV_HIP(c, d.reserve(bytes + 1u, align256(bytes + 1u)));  // (+ 1: items = 0 still gets a buffer, so that the launcher and not a null pointer refuses it)
    if (what == 0) DXV_HIP(c, work.reserve(lanes * blocks + 2u, align256((lanes * blocks + 2u) * sizeof(unsigned long long))));
    hipError_t e = d.p && bytes ? hipMemcpyAsync(d.p, host, bytes, hipMemcpyHostToDevice, s) : hipSuccess;
    unsigned long long* sums = reinterpret_cast<unsigned long long*>(d.p);
    unsigned long long* dTotals = what == 0 ? work.p + lanes * blocks : sums ? sums + n : nullptr;
    if (e == hipSuccess) e = what == 0 ? launch_scan_words(reinterpret_cast<uint32_t*>(d.p), lanes, items, work.p, dTotals, s) : launch_scan_sums(sums, lanes, (uint32_t)items, dTotals, s);
    if (e == hipSuccess) e = hipMemcpyAsync(totals, dTotals, lanes * sizeof(unsigned long long), hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipMemcpyAsync(host, d.p, bytes, hipMemcpyDeviceToHost, s);
    const hipError_t drained = hipStreamSynchronize(s);                 // (the buffers are freed when this returns)
    if (e == hipSuccess) e = drained;
    if (e != hipSuccess) return fail(c, "dxv_debug_scan failed: %s", hipGetErrorString(e));
    return 0;
}

extern "C" int dxv_debug_download(dxv_ctx* c, int what, void* host, size_t bytes)
{
    if (!c || !host) return 1;
#if defined(DXV_PHASE_TIMES)
    if (what == 101 || what == 102) {                                   // the lists kernel's phase sums (102: and reset); diagnostic build only
        if (bytes != 16 * sizeof(unsigned long long)) return fail(c, "dxv_debug_download: phase times are 128 bytes");
        DXV_HIP(c, hipSetDevice(c->device));
        if (sync_frames(c)) return 1;
        DXV_HIP(c, hipDeviceSynchronize());
        DXV_HIP(c, phase_times_read(static_cast<unsigned long long*>(host), what == 102));
        return 0;
    }
#endif
    const void* src = nullptr;
    size_t want = 0;
    const size_t T = c->T;
    hipStream_t s = c->stream;
    if (settle_lists(c)) return 1;
    if ((what == DXV_DBG_NODES || what == DXV_DBG_NODES32 || what == DXV_DBG_NODES64) && c->haveScene && ensure_nodes(c, c->stream)) return 1;
    switch (what) {
    case DXV_DBG_SORTED_KEYS: src = c->scratch.keys.p; want = sizeof(uint64_t) * T; if (c->scratch.T != c->T) src = nullptr; break;
    case DXV_DBG_PARENTS: src = c->scratch.parents.p; want = sizeof(uint32_t) * (2 * T - 1); if (c->scratch.T != c->T) src = nullptr; break;
    case DXV_DBG_NODES: if (c->haveScene) { src = scene_nodes(c); want = sizeof(Node) * (size_t)c->hdr.numNodes; } break;
    case DXV_DBG_NODES32: if (c->haveScene) { src = scene_nodes32(c); want = sizeof(Node32) * (size_t)c->hdr.numNodes; } break;
    case DXV_DBG_NODES64: if (c->haveScene && c->hdr.hasWide) { src = scene_nodes64(c); want = sizeof(Node64) * (size_t)c->hdr.numNodes; } break;
    case DXV_DBG_TRI_POS: if (c->haveScene) { src = scene_tripos(c); want = sizeof(TriPos) * T; } break;
    case DXV_DBG_TRI_NRM: if (c->haveScene) { src = scene_trinrm(c); want = sizeof(TriNrm) * T; } break;
    case DXV_DBG_LIST_CELLS: if (c->haveScene && c->lists.state == 1) { src = c->lists.cells.p; want = sizeof(DirCell) * 6 * (size_t)c->lists.res * c->lists.res; } break;
    case DXV_DBG_LIST_ENTRIES: if (c->haveScene && c->lists.state == 1) { src = c->lists.entries.p; want = sizeof(DirEntry) * (size_t)c->lists.count; } break;
    case DXV_DBG_LIST_MIP: if (c->haveScene && c->lists.state == 1 && c->lists.mip.p) { src = c->lists.mip.p; want = sizeof(uint16_t) * (size_t)dm_mip_words(c->lists.res); } break;
    case DXV_DBG_LIST_STARTS: if (c->haveScene && c->lists.state == 1 && c->lists.starts.p) { src = c->lists.starts.p; want = sizeof(uint32_t) * 6 * (size_t)c->lists.res * c->lists.res; } break;
    case DXV_DBG_LIST_START_CELLS: if (c->haveScene && c->lists.state == 1 && c->lists.startCells.p) { src = c->lists.startCells.p; want = sizeof(DirCell) * 6 * (size_t)c->lists.res * c->lists.res; } break;
    case DXV_DBG_BRICK_EMPTY:
    case DXV_DBG_BRICK_SUMMARY: {                                    // (written on the frame's stream by its last render with flags: launch_raycast)
        const Frame& f = cur_frame(c);
        if (!f.emptyDim || !f.empty.p) return fail(c, "dxv_debug_download: frame %u has not been rendered with empty-brick flags (option skipempty = 1)", c->cur);
        if (f.emptyDim != f.grid_dim) return fail(c, "dxv_debug_download: frame %u's flags are of a %u^3 grid, its grid is %u^3 now (render it again)", c->cur, f.emptyDim, f.grid_dim);
        const size_t M = (f.emptyDim + kEmptyBrick - 1) / kEmptyBrick;
        src = f.empty.p + (what == DXV_DBG_BRICK_SUMMARY ? empty_brick_bytes(f.emptyDim) / 2 : 0);      // (the summaries: the scratch's second half)
        want = M * M * M;
        s = cur_stream(c);
        break;
    }
#if defined(DXV_QUEUE_TIMES)
    case 100: src = c->frames[c->cur].redo.p; want = sizeof(uint64_t) * kRedoCap; break;      // per-wave start / end ticks of the last queue launch
#endif
    default: return fail(c, "dxv_debug_download: unknown selector %d", what);
    }
    if (!src) return fail(c, "dxv_debug_download: selector %d not available", what);
    if (bytes != want) return fail(c, "dxv_debug_download: expected %zu bytes, got %zu", want, bytes);
    DXV_HIP(c, hipSetDevice(c->device));
    DXV_HIP(c, hipMemcpyAsync(host, src, bytes, hipMemcpyDeviceToHost, s));
    DXV_HIP(c, hipStreamSynchronize(s));
    return 0;
}
