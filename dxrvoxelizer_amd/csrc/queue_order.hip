// queue_order.hip -- the order of a PREPARED work queue (dxv_prepare_launch*): direction-major, map tiles dealt to the XCDs.
// k_plan_bricks (plan_bricks.hip) decides WHICH bricks are queued and leaves them in Morton order of voxel space; the order is not
// part of the result, and for a queue that is built once and launched many times it is worth a sort:
//  * the lists a brick reads are indexed by DIRECTION.  All bricks on one radial corridor read the same texels' cells, entries and
//    triangles; in voxel-space Morton order the regions of one corridor run at unrelated times on different XCDs, and every one of
//    them fetches the corridor's data into that XCD's L2 again;
//  * here every queued brick gets a 64-bit key -- class (heavy first) | queue | direction tile of the brick's centre | start radius
//    of the centre (half bits) | brick word -- and the keys are sorted (radix_sort.hip; the brick word is the key's low bits: no
//    values).  A direction tile is 2^T x 2^T texels of one cube-map face (kOrderTileBits), numbered face-major, 2-D Morton inside a
//    face; the tiles that hold a queued brick are dealt round-robin, in that order, to the eight queues -- whole tiles, so that a
//    tile's data lives in ONE XCD's L2 -- and a queue runs its tiles one after the other, every tile from the centre outwards;
//  * the slots are then rewritten from the sorted keys, heavy bricks from slot 0 upwards and the others from the far end downwards
//    exactly as k_plan_bricks lays them out (queue_slot), with the sixteen counts to match.  The set of bricks -- the live mask, the
//    clear -- does not change; the brick kernels do not know the difference.
// Queues that are built inside a launch (and kept ones) keep the Morton order: a sort in every launch costs more than it returns.
#include "dxv_brick.h"
#include "dxv_dirmap.h"

namespace dxv {

#if !defined(DXV_ORDER_TILE_BITS)
#define DXV_ORDER_TILE_BITS 4
#endif
constexpr uint32_t kOrderTileBits = DXV_ORDER_TILE_BITS;               // T: a direction tile is 2^T x 2^T texels (A/B of 3, 4, 5: profiles/NOTES.md)
constexpr uint32_t kOrderTileSideBits = 6u;                             // at most 64 x 64 tiles per face (maps beyond 2^(6 + T) texels: coarser tiles) ...
constexpr uint32_t kOrderTileSlots = 8u << (2u * kOrderTileSideBits);   // ... so a tile number (face << 12 | Morton) is below 2^15
constexpr int kOrderRadiusAt = 30, kOrderTileAt = 45, kOrderQueueAt = 60, kOrderClassAt = 63;   // the key's fields above the 30-bit brick word

struct OrderLens { uint32_t len[8], heavy[8]; };                        // items per queue, of which heavy (as QueueLens, voxelize_lists.hip)

__device__ __forceinline__ uint32_t part1by1(uint32_t x)
{
    x &= 0x0000ffffu;
    x = (x | (x << 8)) & 0x00ff00ffu;
    x = (x | (x << 4)) & 0x0f0f0f0fu;
    x = (x | (x << 2)) & 0x33333333u;
    x = (x | (x << 1)) & 0x55555555u;
    return x;
}
// (tile << 15 | start radius) of the centre of brick word w: dm_ray_point + dm_texel, the functions the kernel's rays go through
__device__ __forceinline__ uint32_t order_tile_radius(const VoxelizeParams& p, uint32_t w)
{
    float x0, x1, y0, y1, z0, z1;
    dm_brick_hull(p.N, p.nz, p.z0, p.zBlock, p.zShift, p.zPeriod, w & 1023u, (w >> 10) & 1023u, w >> 20, x0, x1, y0, y1, z0, z1);
    uint32_t face;
    float u, v, rho;
    dm_ray_point(0.5f * (x0 + x1), 0.5f * (y0 + y1), 0.5f * (z0 + z1), face, u, v, rho);
    const uint32_t R = p.scene.dmR;
    uint32_t sh = kOrderTileBits;
    while ((R >> sh) > (1u << kOrderTileSideBits)) ++sh;
    // (a brick round the grid's very centre has no direction: dm_texel makes texel 0 of whatever the quotients are)
    const uint32_t tile = (face << (2u * kOrderTileSideBits)) | part1by1(dm_texel(u, R) >> sh) | (part1by1(dm_texel(v, R) >> sh) << 1);
    return (tile << 15) | (uint32_t)(half_down(rho) & 0x7fffu);
}
// item i of the queues as k_plan_bricks left them, counted queue after queue: its queue's slot and class
__device__ __forceinline__ uint32_t order_item_word(const VoxelizeParams& p, const OrderLens& lens, uint32_t i, bool& heavy)
{
    uint32_t x = 0;
    while (x < 7u && i >= lens.len[x]) { i -= lens.len[x]; ++x; }
    heavy = i < lens.heavy[x];
    return p.queueSlots[(size_t)x * p.queueCap + queue_slot(i, lens.heavy[x], p.queueCap)];
}

// keys without their queue, and the tiles that are there
__global__ __launch_bounds__(256) void k_order_keys(VoxelizeParams p, OrderLens lens, uint32_t n, uint64_t* __restrict__ keys, uint32_t* __restrict__ present)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    bool heavy;
    const uint32_t w = order_item_word(p, lens, i, heavy), tr = order_tile_radius(p, w);
    keys[i] = ((uint64_t)(heavy ? 0u : 1u) << kOrderClassAt) | ((uint64_t)tr << kOrderRadiusAt) | w;
    present[tr >> 15] = 1u;
}
// ... the queue of every key's tile: its number among the tiles that are there, mod 8; counts[class << 3 | queue] = the keys of each
__global__ __launch_bounds__(256) void k_order_deal(uint32_t n, uint64_t* __restrict__ keys, const uint32_t* __restrict__ ordinal, uint32_t* __restrict__ counts)
{
    __shared__ uint32_t cnt[16];
    if (threadIdx.x < 16u) cnt[threadIdx.x] = 0u;
    __syncthreads();
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i < n) {
        uint64_t k = keys[i];
        const uint32_t x = ordinal[(uint32_t)(k >> kOrderTileAt) & (kOrderTileSlots - 1u)] & 7u;
        k |= (uint64_t)x << kOrderQueueAt;
        keys[i] = k;
        atomicAdd(cnt + (uint32_t)(k >> kOrderQueueAt), 1u);
    }
    __syncthreads();
    if (threadIdx.x < 16u && cnt[threadIdx.x]) atomicAdd(counts + threadIdx.x, cnt[threadIdx.x]);
}
// sorted key i -> its slot: the (i - first key of its class and queue)-th of that class in that queue; the sixteen counts -> the header
struct OrderStarts { uint32_t first[16]; };
__global__ __launch_bounds__(256) void k_order_write(VoxelizeParams p, OrderLens lens, OrderStarts st, uint32_t n, const uint64_t* __restrict__ keys)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i < 8u) { p.queue[queue_heavy_word(i)] = lens.heavy[i]; p.queue[queue_len_word(i)] = lens.len[i] - lens.heavy[i]; }
    if (i >= n) return;
    const uint64_t k = keys[i];
    const uint32_t cat = (uint32_t)(k >> kOrderQueueAt), x = cat & 7u, rank = i - st.first[cat];
    const uint32_t slot = cat < 8u ? rank : p.queueCap - 1u - rank;
    p.queueSlots[(size_t)x * p.queueCap + slot] = (uint32_t)k & 0x3fffffffu;
}

static uint8_t* order_carve(uint8_t*& at, size_t bytes)
{
    uint8_t* here = at;
    at += (bytes + 255u) & ~(size_t)255u;
    return here;
}
struct OrderScratch { uint64_t* keys; uint64_t* tmp; uint32_t* hist; uint32_t* present; uint32_t* ordinal; uint32_t* sums; uint32_t* counts; };
static size_t order_scratch(uint8_t* base, uint32_t n, OrderScratch& o)
{
    uint8_t* at = base;
    o.keys = reinterpret_cast<uint64_t*>(order_carve(at, sizeof(uint64_t) * (size_t)n));
    o.tmp = reinterpret_cast<uint64_t*>(order_carve(at, sizeof(uint64_t) * (size_t)n));
    o.hist = reinterpret_cast<uint32_t*>(order_carve(at, sizeof(uint32_t) * (size_t)radix_sort_hist_words(n)));
    o.present = reinterpret_cast<uint32_t*>(order_carve(at, sizeof(uint32_t) * kOrderTileSlots));
    o.counts = reinterpret_cast<uint32_t*>(order_carve(at, sizeof(uint32_t) * 16u));      // (behind the tiles' words: one memset)
    o.ordinal = reinterpret_cast<uint32_t*>(order_carve(at, sizeof(uint32_t) * kOrderTileSlots));
    o.sums = reinterpret_cast<uint32_t*>(order_carve(at, sizeof(uint32_t) * (kOrderTileSlots / 1024u + 2u)));
    return (size_t)(at - base);
}
size_t queue_order_scratch_bytes(uint32_t n)
{
    OrderScratch o;
    return order_scratch(nullptr, n, o);
}
static void order_lens(const uint32_t lens16[16], OrderLens& lens)
{
    for (int a = 0; a < 8; ++a) { lens.len[a] = lens16[a]; lens.heavy[a] = lens16[8 + a]; }
}

// The n (> 0) bricks of the queue k_plan_bricks built (p.queueSlots, p.queueCap; lens16: its eight lengths, of which heavy) as sorted keys
// in the scratch: *sorted; *counts: sixteen device words, the heavy bricks of the eight new queues, then the others.
hipError_t queue_order_sort(const VoxelizeParams& p, const uint32_t lens16[16], uint32_t n, uint8_t* scratch, const uint64_t** sorted, const uint32_t** counts, hipStream_t s)
{
    OrderScratch o;
    (void)order_scratch(scratch, n, o);
    OrderLens lens;
    order_lens(lens16, lens);
    hipError_t e = hipMemsetAsync(o.present, 0, (size_t)(reinterpret_cast<uint8_t*>(o.counts + 16) - reinterpret_cast<uint8_t*>(o.present)), s);
    if (e != hipSuccess) return e;
    const uint32_t blocks = (n + 255u) / 256u;
    k_order_keys<<<dim3(blocks), dim3(256), 0, s>>>(p, lens, n, o.keys, o.present);
    if ((e = scan_exclusive(o.present, kOrderTileSlots, o.sums, o.ordinal, s)) != hipSuccess) return e;
    k_order_deal<<<dim3(blocks), dim3(256), 0, s>>>(n, o.keys, o.ordinal, o.counts);
    uint64_t* result = nullptr;
    if ((e = radix_sort_keys_bits(o.keys, o.tmp, n, o.hist, 0, 64, &result, s)) != hipSuccess) return e;
    *sorted = result;
    *counts = o.counts;
    return hipGetLastError();
}
// The slots of p.queueSlots (eight queues of p.queueCap words, each able to hold its new length) and the counts of the header p.queue
// (all zero) from the sorted keys; lens16: the NEW eight lengths, of which heavy.
hipError_t queue_order_write(const VoxelizeParams& p, const uint32_t lens16[16], uint32_t n, const uint64_t* sorted, hipStream_t s)
{
    OrderLens lens;
    order_lens(lens16, lens);
    OrderStarts st;
    uint32_t at = 0;
    for (int a = 0; a < 8; ++a) { st.first[a] = at; at += lens.heavy[a]; }
    for (int a = 0; a < 8; ++a) { st.first[8 + a] = at; at += lens.len[a] - lens.heavy[a]; }
    k_order_write<<<dim3((n + 255u) / 256u), dim3(256), 0, s>>>(p, lens, st, n, sorted);
    return hipGetLastError();
}

// ---------------------------------------------------------------------------------------------
// Test hook (dxv_debug_queue_order): what the order promises, read back from the queue as it stands (header p.queue, slots).
// out[0] queued items; out[1] direction tiles that appear in more than one queue within the queues' own first ceil(total / 8) items --
// what an XCD runs before the equal-share spill (queue_item) -- (must be 0); out[2] neighbouring items of one class of one queue whose
// (tile, radius) falls (must be 0); out[3] a wrapping sum over (queue, item, brick word): two builds of one queue give the same.  tiles:
// kOrderTileSlots words of scratch.  Not a product path.
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_order_check(VoxelizeParams p, uint32_t* __restrict__ tiles, unsigned long long* __restrict__ out)
{
    uint32_t heavy[8], len[8], total = 0;
    for (uint32_t x = 0; x < 8u; ++x) { heavy[x] = p.queue[queue_heavy_word(x)]; len[x] = heavy[x] + p.queue[queue_len_word(x)]; total += len[x]; }
    const uint32_t share = (total + 7u) / 8u;
    for (uint32_t x = 0; x < 8u; ++x) {
        for (uint32_t k = blockIdx.x * 256u + threadIdx.x; k < len[x]; k += gridDim.x * 256u) {
            const uint32_t w = p.queueSlots[(size_t)x * p.queueCap + queue_slot(k, heavy[x], p.queueCap)], tr = order_tile_radius(p, w);
            atomicAdd(out, 1ull);
            atomicAdd(out + 3, ((unsigned long long)w + 1ull) * (8ull * k + x + 1ull) * 0x9e3779b97f4a7c15ull);
            if (k < share) atomicOr(tiles + (tr >> 15), 1u << x);
            if (k + 1u < len[x] && (k < heavy[x]) == (k + 1u < heavy[x]) &&
                order_tile_radius(p, p.queueSlots[(size_t)x * p.queueCap + queue_slot(k + 1u, heavy[x], p.queueCap)]) < tr)
                atomicAdd(out + 2, 1ull);
        }
    }
}
__global__ __launch_bounds__(256) void k_order_check_tiles(const uint32_t* __restrict__ tiles, unsigned long long* __restrict__ out)
{
    const uint32_t t = blockIdx.x * 256u + threadIdx.x;
    if (t < kOrderTileSlots && __builtin_popcount(tiles[t]) > 1) atomicAdd(out + 1, 1ull);
}
size_t queue_order_check_words() { return kOrderTileSlots; }
hipError_t launch_queue_order_check(const VoxelizeParams& p, uint32_t* tiles, unsigned long long* out, hipStream_t s)
{
    hipError_t e = hipMemsetAsync(tiles, 0, sizeof(uint32_t) * kOrderTileSlots, s);
    if (e == hipSuccess) e = hipMemsetAsync(out, 0, 4 * sizeof(unsigned long long), s);
    if (e != hipSuccess) return e;
    k_order_check<<<dim3(256), dim3(256), 0, s>>>(p, tiles, out);
    k_order_check_tiles<<<dim3(kOrderTileSlots / 256u), dim3(256), 0, s>>>(tiles, out);
    return hipGetLastError();
}

} // namespace dxv
