// plan_bricks.hip -- the work queue of the lists kernel: which 4 x 4 x 4 bricks a launch runs, built on the device (k_plan_bricks),
// and the launch's zeros that travel with the build (plan_clear; as a kernel of its own: k_clear_grid).  The kernels that run the
// queue: voxelize_lists.hip.
#include "dxv_brick.h"
#include "dxv_dirmap.h"

namespace dxv {

// ---------------------------------------------------------------------------------------------
// Work queue of the lists kernel (4 x 4 x 4 bricks): WHICH bricks a launch runs, decided on the device inside the stream.
//  * which: a ray that starts beyond the last entry of its texel (or whose texel is empty, or whose origin has left the
//    root box) is a miss after one load -- on torus-1M four waves in ten of a launch over the brick box held no other
//    ray.  k_plan_bricks decides per BRICK, conservatively (dm_box_may_be_live, dxv_dirmap.h: the brick's footprint in
//    direction space and its smallest start radius against a max-mip of the texels' far radii; a false positive costs a
//    wave that finds nothing, a false negative cannot happen -- k_plan_check, dxv_debug.hip, is the exhaustive proof obligation);
//  * layout: regions of 256 consecutive bricks of the Morton order (8 x 8 x 4 bricks) are dealt round-robin to eight
//    queues, one per XCD (blocks b and b + 8 share one), so that an XCD's private L2 sees compact regions; a region's
//    workgroup appends its live bricks to its queue with one atomic add (small partitions: runs of 128 bricks, one add per
//    wave -- k_plan_bricks).  Queue memory (dxv_device.h): two headers -- eight heads per queue and the eight lengths, every
//    word in a 256-byte line of its own; a build takes the one the last build left cleared -- and 8 x cap brick words
//    (bx | by << 10 | bz << 20);
//  * how: k_voxelize_queue is launched with as many single-wave workgroups as the GPU holds at once.  Every wave takes its
//    bricks one at a time from a head of its XCD's queue with a returning atomic add, asked for one brick ahead.  Which
//    XCD a block really runs on is a matter of speed only: every head of every queue has its home waves by block number.
//    No host round trip: the launch's size does not depend on how many bricks are live.
//  * order: TWO orders.  A queue that a launch builds for itself (and a kept one) runs as built -- Morton order of voxel space, regions
//    dealt round-robin.  A PREPARED queue (dxv_prepare_launch*, built once and launched many times) is sorted after this build into
//    direction-major order -- heavy first, then by the direction tile of the brick's centre and its start radius, whole tiles dealt
//    round-robin to the eight queues: queue_order.hip -- because the lists are indexed by direction: an XCD's L2 then fetches a
//    corridor's cells, entries and triangles once per launch, not once per region along the radius (torus-1M at 512^3: 718 -> 282 MB
//    fetched per launch, L2 hit rate 84 -> 90 %, the kernel -6 %).  Same bricks, same layout (queue_slot), same live mask.
//    Measured and dropped for the order as built (profiles/r04/ab_queue_*): dealing finer or to
//    the shortest queue; a second queue per XCD, run last, for the bricks near or across the outer end of their lists (three
//    definitions); and, for queues that are launched again, orders made on the device from MEASURED times -- the cheapest chunks of
//    64 slots last (-3 % of a rank's share, +1 % on a whole grid), all chunks by cost (-6 % / +4 %), the bricks that took over three
//    times the mean first and the shortest last (nothing): none earns a second copy of the queue.
// Bricks that are not queued are zero because k_plan_bricks clears the partition's grid while it builds the queue.
// ---------------------------------------------------------------------------------------------
constexpr uint32_t kPlanRegionBits = 8u;                               // regions of 256 consecutive bricks = one workgroup of k_plan_bricks
// (header layout: queue_len_word / queue_head_word in dxv_device.h -- every queue's two words in a 256-byte line of its own:
// returning atomics on ONE line serialise at ~90 per us for all eight queues together, 2.7 ms of a launch when first tried)

// The launch's zeros travel with the queue build: workgroup b clears the b-th share of the grid (and of the texel image) with
// 16-byte stores while its threads wait for their four mip words -- one kernel in front of the brick kernel instead of a memset
// of the grid, a memset of the header and this one (three dependent dispatches: ~5 us each on top of their own time).
// Block 0 clears the frame's other header for the launch that builds the next queue.
__device__ __forceinline__ void plan_clear(uint8_t* base, size_t bytes, uint32_t nblocks)
{
    const size_t chunk = (((bytes + nblocks - 1u) / nblocks) + 15u) & ~(size_t)15u;
    const size_t lo = (size_t)blockIdx.x * chunk;
    if (lo >= bytes) return;
    const size_t hi = lo + chunk < bytes ? lo + chunk : bytes, full = lo + ((hi - lo) & ~(size_t)15u);
    // (non-temporal stores: 134 MB of zeros that nobody reads before the brick kernel has overwritten a fifth of them should not push
    // the lists out of the L2s and the memory-side cache on their way -- plain stores: the queue build 0.0375 instead of 0.0328 ms and
    // the brick kernel behind it 0.681 instead of 0.666, profiles/r05/ab_nontemporal_grid_stores.jsonl)
    typedef uint32_t Zero4 __attribute__((ext_vector_type(4)));
    const Zero4 z = {0u, 0u, 0u, 0u};
    for (size_t o = lo + 16u * threadIdx.x; o < full; o += 16u * 256u) __builtin_nontemporal_store(z, reinterpret_cast<Zero4*>(base + o));
    if (full + threadIdx.x < hi) base[full + threadIdx.x] = 0;           // (a grid whose bytes are no multiple of 16: the last block's tail)
}

__global__ __launch_bounds__(256) void k_plan_bricks(VoxelizeParams p, uint32_t nb)
{
    __shared__ uint32_t heavyCount[4], lightCount[4], heavyBase[4], lightBase[4];
    const uint32_t lin = blockIdx.x * 256u + threadIdx.x, lane = threadIdx.x & 63u, w = threadIdx.x >> 6;
    bool live = false;
    uint32_t bx = 0, by = 0, bz = 0;
    float x0 = 0.0f, x1 = 0.0f, y0 = 0.0f, y1 = 0.0f, z0 = 0.0f, z1 = 0.0f;    // the brick's hull: for `live` here, for `heavy` below
    if (lin < nb) {
        brick_of_lin(p, lin, bx, by, bz);
        dm_brick_hull(p.N, p.nz, p.z0, p.zBlock, p.zShift, p.zPeriod, bx, by, bz, x0, x1, y0, y1, z0, z1);
        live = dm_box_may_be_live(x0, x1, y0, y1, z0, z1, p.scene.rootLo, p.scene.rootHi, p.mip, p.scene.dmR);
    }
    if (p.planClear) {
        plan_clear(p.grid, (size_t)p.N * p.N * p.nz, gridDim.x);
        if (p.texels) plan_clear(reinterpret_cast<uint8_t*>(p.texels), (size_t)p.N * p.N * p.nz * 4u, gridDim.x);
    }
    if (p.queueZero && blockIdx.x == 0u)
        for (uint32_t k = threadIdx.x; k < kQueueHeaderWords; k += 256u) p.queueZero[k] = 0u;
    // heavy: one of the brick's rays can look into a list that is long for this scene (one and a half times the mean of the count
    // mip at the level of a brick's patch of texels: k_dm_heavy_thresholds) -- 2 - 6 % of the queued bricks, among them 99 % of those
    // that take three times the mean and more (profiles/r05/brick_features.jsonl)
    bool heavy = false;
    if (live) {
        const uint16_t* countMip = p.mip + dm_mip_words(p.scene.dmR);
        // (maps too small to have such a level -- R < 8 -- have no word: no brick is heavy there)
        const uint32_t longList = p.planHeavy ? p.planHeavy : dm_mip_levels(p.scene.dmR) > kDmHeavyLevelMin ? countMip[dm_mip_words(p.scene.dmR) + dm_heavy_level(p.scene.dmR, p.N)] : 0xffffu;
        heavy = dm_box_max_count(x0, x1, y0, y1, z0, z1, countMip, p.scene.dmR) > longList;
    }
    const unsigned long long mh = __ballot(live && heavy), ml = __ballot(live && !heavy);
    if (lane == 0u) { heavyCount[w] = (uint32_t)__builtin_popcountll(mh); lightCount[w] = (uint32_t)__builtin_popcountll(ml); }
    __syncthreads();
    // Runs of 2^planRegionBits consecutive Morton bricks go to one queue, the runs dealt round-robin: 256 (8 x 8 x 4 bricks, the whole
    // workgroup: an XCD's L2 sees compact pieces of the grid), 128 or 64 (one wave each).
    const uint32_t wavesPerRun = 1u << (p.planRegionBits - 6u), first = w & ~(wavesPerRun - 1u);
    const uint32_t x = (lin >> p.planRegionBits) & 7u;
    if (lane == 0u && w == first) {
        uint32_t nh = 0, nl = 0;
        for (uint32_t k = 0; k < wavesPerRun; ++k) { nh += heavyCount[first + k]; nl += lightCount[first + k]; }
        heavyBase[first] = nh ? atomicAdd(p.queue + queue_heavy_word(x), nh) : 0u;
        lightBase[first] = nl ? atomicAdd(p.queue + queue_len_word(x), nl) : 0u;
    }
    __syncthreads();
    if (!live) return;
    const unsigned long long before = (1ull << lane) - 1ull;
    uint32_t rank = (uint32_t)__builtin_popcountll((heavy ? mh : ml) & before);
    for (uint32_t k = first; k < w; ++k) rank += heavy ? heavyCount[k] : lightCount[k];
    // (heavy bricks from slot 0 upwards, the others from the far end downwards: queue_slot)
    const uint32_t slot = heavy ? heavyBase[first] + rank : p.queueCap - 1u - (lightBase[first] + rank);
    p.queueSlots[(size_t)x * p.queueCap + slot] = bx | (by << 10) | (bz << 20);
    if (p.liveMask) {                                                   // (a queue that is being prepared: the bit the launches' clear reads)
        const uint32_t nbx = (p.N + 3u) / 4u, id = (bz * nbx + by) * nbx + bx;
        atomicOr(p.liveMask + (id >> 5), 1u << (id & 31u));
    }
}
size_t plan_live_words(uint32_t N, uint32_t nz)
{
    const uint64_t nbx = (N + 3u) / 4u, nbz = (nz + 3u) / 4u;
    return (size_t)((nbx * nbx * nbz + 31u) / 32u) + 4u;
}

// the brick order of the whole partition (no brick box): what k_plan_bricks, the checker and the host agree on
uint32_t plan_layout(VoxelizeParams& p)
{
    const uint32_t nbx = (p.N + 3u) / 4u, nby = nbx, nbz = (p.nz + 3u) / 4u;
    p.nbx = nbx; p.nby = nby; p.nbz = nbz;
    p.bx0 = p.by0 = p.bz0 = 0;
    uint32_t m = 0;
    while (m < 10 && !((nbx >> m) & 1u) && !((nby >> m) & 1u) && !((nbz >> m) & 1u)) ++m;
    p.mortonBits = m;
    p.superX = nbx >> m;
    p.superY = nby >> m;
    return nbx * nby * nbz;
}
// Run length by partition size.  Large partitions: 256 bricks (an XCD's L2 sees compact pieces of the grid, and with thousands of
// runs per queue the eight queues end within 2 % of each other).  Small ones -- a 256^3 grid, a rank's share of 512^3 at 4 ranks
// or more: 2^19 bricks or fewer -- take shorter runs: a queue of a few hundred runs of very different cost ends 10 - 20 % away
// from its neighbours, and the launch ends with the longest.  (Runs of 64 until round 6; since every XCD runs an equal share of all
// eight queues -- queue_item -- their imbalance matters less than an XCD's locality: 128 is -3 % at 256^3 and -2 ... -3 % on a
// rank's share of the 1 M-triangle meshes at 512^3, +1.5 % on dragon x9's: profiles/r06/ab_planregion_at_eight_waves.jsonl.)
uint32_t plan_region_bits(uint32_t N, uint32_t nz)
{
    const uint64_t nb = (uint64_t)((N + 3u) / 4u) * ((N + 3u) / 4u) * ((nz + 3u) / 4u);
    return nb <= (1ull << 19) ? 7u : kPlanRegionBits;
}
// words of queue memory a partition needs (two headers + eight queues, each able to hold every run dealt to it in full, whatever
// the run length)
size_t plan_queue_words(uint32_t N, uint32_t nz, uint32_t* capOut)
{
    const uint64_t nb = (uint64_t)((N + 3u) / 4u) * ((N + 3u) / 4u) * ((nz + 3u) / 4u);
    uint64_t cap = 0;
    for (uint32_t rb = 6u; rb <= kPlanRegionBits; ++rb) {
        const uint64_t runs = (nb + (1u << rb) - 1u) >> rb, c = ((runs + 7u) / 8u) << rb;
        if (c > cap) cap = c;
    }
    if (capOut) *capOut = (uint32_t)cap;
    return kQueueSlotsAt + 8u * (size_t)cap;
}

// one workgroup per 256 bricks into the header p.queue, which the caller vouches is all zero; p.queueSlots / p.queueCap / p.mip set by the caller
hipError_t plan_build(const VoxelizeParams& pin, hipStream_t s)
{
    VoxelizeParams p = pin;
    const uint32_t nb = plan_layout(p), nr = (nb + (1u << kPlanRegionBits) - 1u) >> kPlanRegionBits;
    if (p.planRegionBits < 6u || p.planRegionBits > kPlanRegionBits) p.planRegionBits = kPlanRegionBits;
    k_plan_bricks<<<dim3(nr), dim3(256), 0, s>>>(p, nb);
    return hipGetLastError();
}

// the clear as a kernel of its own (a launch through a prepared queue with clearMode 0, and every grid whose side is no multiple of 16:
// launch_voxelize_prepared, voxelize_lists.hip): the whole partition
__global__ __launch_bounds__(256) void k_clear_grid(VoxelizeParams p)
{
    plan_clear(p.grid, (size_t)p.N * p.N * p.nz, gridDim.x);
    if (p.texels) plan_clear(reinterpret_cast<uint8_t*>(p.texels), (size_t)p.N * p.N * p.nz * 4u, gridDim.x);
}
hipError_t plan_clear_grid(const VoxelizeParams& p, hipStream_t s)
{
    // (about one workgroup of 256 threads per 64 KiB, at least 8 and at most 8,192)
    uint32_t nb = (uint32_t)(((size_t)p.N * p.N * p.nz + 65535u) >> 16);
    nb = nb < 8u ? 8u : nb > 8192u ? 8192u : nb;
    k_clear_grid<<<dim3(nb), dim3(256), 0, s>>>(p);
    return hipGetLastError();
}

} // namespace dxv
