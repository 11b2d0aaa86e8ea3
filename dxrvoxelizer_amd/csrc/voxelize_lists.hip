// voxelize_lists.hip -- the reference rule through the direction-space lists: the two brick kernels that run the work queue of live
// 4 x 4 x 4 bricks (k_voxelize_queue: persistent waves; k_voxelize_listed: one workgroup per queued brick) -- the product's hot path --
// and the equal shares they take of it.  The queue itself and how it is built: plan_bricks.hip.  The same brick body over a brick box,
// without a queue: k_voxelize<..., WALK 4>, traverse.hip.
#include "dxv_brick.h"
#include "dxv_dirmap.h"
#include <algorithm>
#include <vector>

namespace dxv {

[[maybe_unused]] constexpr uint32_t kQueueNoPrefetch = 1024u;

// ---------------------------------------------------------------------------------------------
// Eight queues of unequal length, eight XCDs of equal appetite.  Runs of bricks are dealt to the queues by their number, not by
// what they hold: on a rank's share of the grid the queues differ by up to 30 % in length (bunny x16 at 8 ranks: 6,400 against
// 9,100 bricks), and a launch ends with its longest queue while half of the GPU idles (profiles/r05/wg_times_before.jsonl).  So
// the launch is dealt out in EQUAL shares: XCD x runs T = ceil(total / 8) items -- its own queue's first min(len_x, T), and, when
// its queue is shorter than T, items from the far end of the queues that are longer (what they hold beyond their own first T), in
// queue order.  A pure function of the eight lengths, which every workgroup reads from the header: no second pass over the
// queues, nothing moved; 85 - 100 % of an XCD's bricks are still its own compact runs.
// ---------------------------------------------------------------------------------------------
struct QueueLens { uint32_t len[8], heavy[8]; };        // items per queue, of which heavy
#if defined(__HIP_DEVICE_COMPILE__)
// (the arithmetic runs on lanes 0 .. 7 of the wave -- one length each -- where a brick body that has not begun yet leaves every
// vector register free; held in scalar registers the eight lengths cost the persistent kernel a wave per SIMD)
__device__ __forceinline__ uint32_t dpp_row_shr(uint32_t v, int n)      // lane i <- lane i - n of its row of 16, 0 where there is none
{
    return n == 1 ? (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x111, 0xf, 0xf, true)
         : n == 2 ? (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x112, 0xf, 0xf, true)
                  : (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x114, 0xf, 0xf, true);
}
__device__ __forceinline__ uint32_t prefix8(uint32_t v)                 // inclusive prefix sums over lanes 0 .. 7 (v = 0 on the lanes behind them)
{
    v += dpp_row_shr(v, 1); v += dpp_row_shr(v, 2); v += dpp_row_shr(v, 4);
    return v;
}
__device__ __forceinline__ uint32_t queue_lens(const uint32_t* hdr, uint32_t& T, uint32_t& H)   // lane a < 8: items of queue a, of which H heavy; T = ceil(total / 8)
{
    const uint32_t lane = lane_id();
    H = lane < 8u ? hdr[queue_heavy_word(0) + 64u * lane] : 0u;
    const uint32_t L = lane < 8u ? hdr[queue_len_word(0) + 64u * lane] + H : 0u;
    T = ((uint32_t)__builtin_amdgcn_readlane((int)prefix8(L), 7) + 7u) >> 3;
    return L;
}
// item j (< T) of XCD x: queue and slot; false: none (the last few of the 8 T items when the total is no multiple of 8)
__device__ __forceinline__ bool queue_item(const uint32_t* hdr, uint32_t cap, uint32_t x, uint32_t j, uint32_t& y, uint32_t& slot)
{
    uint32_t T, H, k;
    const uint32_t L = queue_lens(hdr, T, H), lenX = (uint32_t)__builtin_amdgcn_readlane((int)L, (int)x);
    if (j < lenX) { y = x; k = j; }                             // (j < T: one of the queue's own first T)
    else {
        const uint32_t lane = lane_id();
        const uint32_t spare = lane < 8u && L < T ? T - L : 0u, extra = L > T ? L - T : 0u;
        const uint32_t spareBefore = prefix8(spare) - spare, extraBefore = prefix8(extra) - extra;
        // the (j - len_x)-th slot this XCD has to spare, counted behind the spare slots of the XCDs 0 .. x - 1, is given the g-th
        // brick that some queue holds beyond its own first T
        const uint32_t g = j - lenX + (uint32_t)__builtin_amdgcn_readlane((int)spareBefore, (int)x);
        const uint64_t m = __builtin_amdgcn_ballot_w64(lane < 8u && g >= extraBefore && g - extraBefore < extra);
        if (!m) return false;
        y = (uint32_t)__builtin_ctzll(m);
        k = T + g - (uint32_t)__builtin_amdgcn_readlane((int)extraBefore, (int)y);
    }
    slot = queue_slot(k, (uint32_t)__builtin_amdgcn_readlane((int)H, (int)y), cap);
    return true;
}
// the same from eight lengths the host holds (a kept queue, k_voxelize_listed: kernel arguments, no load in front of the brick's own)
__device__ __forceinline__ bool queue_item(const QueueLens& q, uint32_t cap, uint32_t x, uint32_t j, uint32_t& y, uint32_t& slot)
{
    uint32_t total = 0, lenX = 0, k = 0;
#pragma unroll
    for (int a = 0; a < 8; ++a) { total += q.len[a]; lenX = x == (uint32_t)a ? q.len[a] : lenX; }
    const uint32_t T = (total + 7u) >> 3;
    bool found = j < lenX;
    y = x; k = j;
    if (!found) {
        uint32_t g = j - lenX;
#pragma unroll
        for (int a = 0; a < 8; ++a) g += ((uint32_t)a < x && q.len[a] < T) ? T - q.len[a] : 0u;
#pragma unroll
        for (int a = 0; a < 8; ++a) {
            const uint32_t extra = q.len[a] > T ? q.len[a] - T : 0u;
            if (!found && g < extra) { y = (uint32_t)a; k = T + g; found = true; }
            g -= found ? 0u : extra;
        }
    }
    uint32_t heavy = 0;
#pragma unroll
    for (int a = 0; a < 8; ++a) heavy = y == (uint32_t)a ? q.heavy[a] : heavy;
    slot = queue_slot(k, heavy, cap);
    return found;
}
#endif

// ---------------------------------------------------------------------------------------------
// The lists kernel over the work queue: persistent single-wave workgroups (see above).  One brick = one pass of the body of
// k_voxelize<Brick<4,4,4>, 16, 0, TEXELS, 4>; the 64 result bytes of a brick leave as 16 dwords (one per 4-voxel row,
// assembled from the wave's ballot) instead of 64 bytes.
// ---------------------------------------------------------------------------------------------
// (the body; STARTS: compiled to read the lists' START CELLS -- the cells with the start table's word in them: dm_ray_start<2>, dxv_dirmap.h --
// or the canonical cells, as if there were no table)
template <bool TEXELS, bool STARTS>
__device__ __forceinline__ void queue_bricks(const VoxelizeParams& p)
{
#if defined(__HIP_DEVICE_COMPILE__)
    __shared__ int32_t stack[16 * 64];
    // A queue is handed out through eight heads: head h counts the slots k = h (mod 8), so that the eight groups of an XCD's waves
    // (a wave's home head: its number among the XCD's waves mod 8) advance through the queue together, one brick per add -- the
    // bricks in flight on an XCD stay a compact window of its queue (what hardware dispatch of one workgroup per brick gave:
    // neighbouring bricks look into the same texels while they are in the caches; chunks of 8 consecutive bricks per wave
    // cost 7 %, of 16 15 %), and no head sees more than a few adds per microsecond (all bricks through ONE word: 2.7 ms).
#if defined(DXV_QUEUE_TIMES)
    const uint64_t tStart = __builtin_amdgcn_s_memrealtime();
    uint64_t tBrick = tStart, tLast = tStart, tMax = 0, nBricks = 0;
#endif
    // Every head has HOME waves that drain it to its last slot: wave w of XCD x (x = block % 8, w = block / 8) is home to the heads
    // h = w (mod 8) of queue x -- to h = w (mod W) when fewer than eight waves per XCD were launched, so that no head is without
    // one (which XCD a block really runs on is a matter of speed only).
    const uint32_t nh = p.queueHeads;                                   // heads per queue in use: 1, 2, 4 or 8 (head h hands out the items = h mod nh)
    const uint32_t x0 = blockIdx.x & 7u, wx = blockIdx.x >> 3;
    uint32_t perXcd = gridDim.x >> 3;
    // A short launch does not want every wave the GPU holds: with fewer than p.queueMinBricks bricks per wave the bricks of a wave
    // contend with seven times as many neighbours as they need to fill the launch's few rounds, and each wave holds one brick in
    // reserve at the end (256^3, 60 k bricks: 0.192 ms with 7,168 waves, 0.166 with 5,120: profiles/r05/ab_persistent_waves.jsonl).
    // The launch cannot know its size on the host; its waves can: the surplus ones leave before they touch the queue.
    if (p.queueMinBricks) {
        uint32_t share, heavy;
        (void)queue_lens(p.queue, share, heavy);
        uint32_t want = ((share + p.queueMinBricks - 1u) / p.queueMinBricks + 7u) & ~7u;      // (a multiple of 8: every head keeps its home waves)
        want = want < 64u ? 64u : want;
        if (want < perXcd) perXcd = want;
        if (wx >= perXcd) return;
    }
    const uint32_t homes = perXcd < nh ? perXcd : nh;
    uint64_t homeMask = 0;
    for (uint32_t h = wx % homes; h < nh; h += homes) homeMask |= 1ull << (8u * x0 + h);
    uint32_t cur = 8u * x0 + wx % homes;
    uint64_t tried = 0;
    for (;;) {
        tried |= 1ull << cur;
        const uint32_t x = cur >> 3, h = cur & 7u;
        uint32_t len, own, ownHeavy;                                    // items of XCD x: its equal share of the launch (queue_item)
        {
            uint32_t H;
            const uint32_t L = queue_lens(p.queue, len, H);
            own = (uint32_t)__builtin_amdgcn_readlane((int)L, (int)x);  // ... of which its own queue's, and how many of those are heavy
            ownHeavy = (uint32_t)__builtin_amdgcn_readlane((int)H, (int)x);
        }
        uint32_t* head = p.queue + queue_head_word(x, h);
        if (len > h) {
        // One brick ahead: the add for the next brick is issued in front of the current one, and its answer is taken out of its
        // vector register as soon as the brick's first load (the rays' cells: all 64 lanes make that step together) has arrived --
        // by then it is there (memory operations return in order) -- so nothing of the queue lives in a vector register through
        // the scan and the triangle tests.
        // (... except near a queue's end: a wave that holds a second brick there keeps it from the waves that have run out of work)
        uint32_t jv = 0;
        if (threadIdx.x == 0u) jv = atomicAdd(head, 1u);
        uint32_t next = (uint32_t)__builtin_amdgcn_readlane((int)jv, 0);
        uint32_t wAhead = 0xffffffffu;                                  // the next brick's word when it was fetched during the current brick (no brick word has its top bits set)
        bool asked = false;                                             // an add is in flight (asked for behind the last brick's scan)
        for (;;) {
            const uint32_t k = nh * next + h;
            if (k >= len) break;
            const bool ahead = len - k > kQueueNoPrefetch;
            if (ahead && !asked && threadIdx.x == 0u) jv = atomicAdd(head, 1u);   // (a head's first brick; later ones: behind the scan of the brick before)
            // The launch's parameters are read from the kernel-argument segment again for every brick (scalar loads that
            // hit the scalar cache): kept across the loop they would hold fifty SGPRs through the whole brick body, and the
            // body (the one of k_voxelize: 70 VGPRs, 56 SGPRs) would lose a wave per SIMD to registers.
            typedef const __attribute__((address_space(4))) VoxelizeParams* KernArg;
            KernArg pp = (KernArg)__builtin_amdgcn_kernarg_segment_ptr();
            asm volatile("" : "+s"(pp));
            uint32_t w = wAhead;                                        // through the scalar cache: one word per wave
            if (w == 0xffffffffu) {
                const uint32_t* hdr = pp->queue;
                const uint32_t cap = pp->queueCap;
                uint32_t qy = x, qslot = queue_slot(k, ownHeavy, cap);
                bool any = true;
                if (k >= own) any = queue_item(hdr, cap, x, k, qy, qslot);      // (beyond the XCD's own queue: a longer queue's far end)
                if (!any) break;                                        // (only the very last items of the launch)
                const uint32_t* slot = pp->queueSlots + (uint32_t)__builtin_amdgcn_readfirstlane((int)(qy * cap + qslot));   // (8 cap <= 2^27 bricks)
                asm volatile("s_load_dword %0, %1, 0x0\n\ts_waitcnt lgkmcnt(0)" : "=s"(w) : "s"(slot) : "memory");
            }
            SceneView sc;                                               // (what the lists' path reads of it)
            sc.nodes = nullptr; sc.wide = nullptr; sc.plCells = nullptr; sc.plEntries = nullptr; sc.plR = 0;
            sc.triPos = pp->scene.triPos; sc.triNrm = pp->scene.triNrm;
            sc.dmCells = pp->scene.dmCells; sc.dmEntries = pp->scene.dmEntries; sc.dmR = pp->scene.dmR; sc.dmCoop = pp->scene.dmCoop; sc.dmStarts = pp->scene.dmStarts;
            sc.dmStartCells = STARTS ? pp->scene.dmStartCells : nullptr;
#pragma unroll
            for (int a = 0; a < 3; ++a) { sc.rootLo[a] = pp->scene.rootLo[a]; sc.rootHi[a] = pp->scene.rootHi[a]; }
            // (the brick's set-up, down to origin_leaves_root: written out once more in k_voxelize_listed -- one helper for both changes both kernels' instruction streams)
            const uint32_t N = pp->N, nz = pp->nz;
            const uint32_t bx = w & 1023u, by = (w >> 10) & 1023u, bz = w >> 20;
            // (the lane number anew for every brick, and once more behind the body: nothing of the loop lives in vector registers
            // through the body)
            uint32_t tid = lane_id();
            uint32_t ix, iy, lz;
            brick_voxel_clamped(N, nz, bx, by, bz, tid, ix, iy, lz);
            // (global_slice, dxv_math.h, written out: called with these operands the helper leaves this kernel one instruction with its operands
            // in another order, and the kernel's instruction stream is kept exactly as it was measured)
            const uint32_t zBlock = pp->zBlock;
            const uint32_t iz = zBlock == nz ? pp->z0 + lz : pp->z0 + (lz >> pp->zShift) * pp->zPeriod + (lz & (zBlock - 1u));
            // raygenMain for the 64 voxels of the brick (voxel_reference<4>, dxv_trace.h, with its first step made by all lanes)
            Ray r;
            ray_origin(N, ix, iy, iz, r.ox, r.oy, r.oz);
            const DirMapView dm{static_cast<const DirCell*>(sc.dmCells), static_cast<const DirEntry*>(sc.dmEntries), sc.dmR, sc.dmCoop, sc.dmStarts, static_cast<const DirCell*>(sc.dmStartCells)};
            DirRayStart start = dm_ray_start<STARTS ? 2 : 0>(r.ox, r.oy, r.oz, dm);
            wAhead = 0xffffffffu;
            if (ahead) {
                next = (uint32_t)__builtin_amdgcn_readlane((int)jv, 0);  // the next brick's number
                // ... and its word, asked for now: fetched at the top of the loop it is a scalar load that nothing hides -- 0.7 us of an
                // 11 us brick, the difference between these waves and a workgroup per brick dealt out by the hardware.  (One scalar
                // register through the body; items beyond the XCD's own queue -- queue_item -- are looked up when their turn comes.)
                const uint32_t kn = nh * next + h;
                if (kn < own) {
                    typedef const __attribute__((address_space(4))) uint32_t* ConstWords;
                    wAhead = ((ConstWords)pp->queueSlots)[x * pp->queueCap + queue_slot(kn, ownHeavy, pp->queueCap)];
                }
            }
            if (origin_leaves_root(r.ox, r.oy, r.oz, sc.rootLo, sc.rootHi)) start.live = false;   // provably missMain
            Hit best;
            float bestDet = 1.0f;
            const StridedStack stk{stack + tid, 64};
            trace_reference_dm_from<StridedStack, 0, TEXELS ? 0 : 2, STARTS ? 2 : 0>(r, dm, start, sc.triPos, stk, 16, best, bestDet);
            // The add for the brick AFTER the next one, here: vector memory answers in order, so an add asked for right in front of a
            // brick's first load makes that load wait for the add's 1.1 - 1.3 us instead of its own 0.8 -- asked for behind the scan,
            // it has the predicate, the stores and the next brick's ray set-up (nine divisions) to come back in.
            asked = false;
            if (ahead) {
                const uint32_t kn = nh * next + h;
                if (kn < len && len - kn > kQueueNoPrefetch) {
                    if (threadIdx.x == 0u) jv = atomicAdd(head, 1u);
                    asked = true;
                }
            }
            uint32_t texel = 0;
            const uint8_t occ = TEXELS ? shade_reference<4, 0>(sc, r, best, bestDet, &texel) : shade_reference_again(sc, r, best.leaf);
            // the lane's voxel once more (nothing of it was kept through the body: store_brick, dxv_brick.h)
            tid = lane_id();
            store_brick<TEXELS>(pp, N, nz, bx, by, bz, tid, occ, texel);
#if defined(DXV_QUEUE_TIMES)
            { const uint64_t now = __builtin_amdgcn_s_memrealtime(); tLast = tBrick; if (now - tBrick > tMax) tMax = now - tBrick; tBrick = now; ++nBricks; }
#endif
            if (!ahead) {
                if (threadIdx.x == 0u) jv = atomicAdd(head, 1u);
                next = (uint32_t)__builtin_amdgcn_readlane((int)jv, 0);
            }
        }
        }
        // this head is done: the wave's other home heads (fewer than eight waves per XCD), else the wave is done.  A wave does NOT go
        // looking for work on other heads or other XCDs' queues: at the end of a launch thousands of waves doing so at once are
        // thousands of adds and loads on single words (~90 per microsecond each) -- measured, in four variants: every wave spent
        // 30 - 60 us there and a rank's share of the grid took 0.195 instead of 0.147 ms (profiles/r04/queue_wave_times.jsonl,
        // ab_queue_helping.jsonl).  Round 5 tried the cheapest form once more -- one load of the wave's own queue's eight heads, then a
        // move to the head with most items left, never to another XCD's queue: a rank's share 0.142 -> 0.170 ms (the waves of a
        // drained head all pick the same head: profiles/r05/ab_steal_within_the_queue_rejected.jsonl, .patch).
        const uint64_t homeLeft = homeMask & ~tried;
        if (!homeLeft) break;
        cur = (uint32_t)__builtin_ctzll(homeLeft);
    }
#if defined(DXV_QUEUE_TIMES)
    // (diagnostic build only, tools/queue_times.py: start and end of every wave in 100 MHz ticks, in the frame's unused redo list)
    if (threadIdx.x == 0u && 4u * blockIdx.x + 3u < p.redoCap) {
        p.redo[4u * blockIdx.x] = tStart; p.redo[4u * blockIdx.x + 1u] = __builtin_amdgcn_s_memrealtime();
        p.redo[4u * blockIdx.x + 2u] = (nBricks << 32) | tMax; p.redo[4u * blockIdx.x + 3u] = tLast;      // bricks, longest brick, start of the last one
    }
#endif
#else
    (void)p;
#endif
}
// ... as kernels: for launches whose lists have a start table the launch reads (through the start cells), and for launches without (_plain)
template <bool TEXELS> __global__ __launch_bounds__(64, 6) void k_voxelize_queue(VoxelizeParams p) { queue_bricks<TEXELS, true>(p); }
template <bool TEXELS> __global__ __launch_bounds__(64, 6) void k_voxelize_queue_plain(VoxelizeParams p) { queue_bricks<TEXELS, false>(p); }

// The same brick body with one workgroup per queued brick, dispatched by the hardware: for a queue that is launched AGAIN and whose
// eight lengths the host has read meanwhile (dxv_sync of an earlier launch of the same queue) -- the launch's size is then
// known without a round trip of its own.  Workgroup b takes item b / 8 of XCD b % 8's equal share (workgroups b and b + 8 share an XCD);
// no heads, no adds, parameters in scalar registers from the start.  What it is for: short launches (a 256^3 grid, a rank's
// share), whose few bricks per persistent wave leave the end of the launch ragged (option dispatch).
// The clear of a launch through a PREPARED queue (launch_voxelize_prepared), inside the brick kernel's own dispatch: the bricks that are
// queued write all 64 of their voxels themselves, so a launch only has to zero the bricks that are NOT queued -- and that has no order
// to keep with the brick workgroups (disjoint bytes), which is what lets both share one dispatch.  One thread per 16 voxels of a grid
// row (16 bytes = four bricks' rows) and step; the four bricks' bits sit in one nibble of the prepared queue's brick mask (ids run
// along x, N % 16 == 0).  Non-temporal stores, like every clear of this file: zeros nobody reads soon should not push the lists out
// of the caches.
struct ClearShare { const uint32_t* live; uint32_t blocks; uint32_t where; };   // blocks: workgroups that clear (0: none, a multiple of 8); where: 1 = the launch's first,
                                                                                // 2 = its last, 3 = spread evenly between the bricks' (rows of 8 workgroups, one per XCD)
__device__ __forceinline__ void clear_dead_bricks(const VoxelizeParams& p, const uint32_t* __restrict__ live, uint32_t block, uint32_t nblocks)
{
    typedef uint32_t Zero4 __attribute__((ext_vector_type(4)));
    const Zero4 z = {0u, 0u, 0u, 0u};
    const uint32_t N = p.N, px = N >> 4, nbx = N >> 2;
    const uint32_t pieces = px * N * p.nz, per = (pieces + nblocks - 1u) / nblocks;      // (<= 2^29 pieces: 32-bit arithmetic throughout)
    const uint32_t lo = block * per, hi = lo + per < pieces ? lo + per : pieces;
    // four pieces per thread and round: their mask words are asked for together (a chain of sixteen dependent loads per thread made
    // a clearing workgroup last 16 us -- longer than a brick)
    for (uint32_t base = lo; base < hi; base += 256u) {                 // (wave-uniform: the texel image's stores read other lanes' nibbles)
        const uint32_t q0 = base + threadIdx.x;
        uint32_t nib[4];
#pragma unroll
        for (uint32_t u = 0; u < 4u; ++u) {
            const uint32_t q = q0 + 64u * u;
            nib[u] = 15u;                                              // (beyond the share: nothing to do)
            if (q < hi) {
                const uint32_t row = q / px, x16 = q - row * px, lz = row / N, y = row - lz * N;
                const uint32_t bit = ((lz >> 2) * nbx + (y >> 2)) * nbx + (x16 << 2);
                nib[u] = (live[bit >> 5] >> (bit & 31u)) & 15u;
            }
        }
#pragma unroll
        for (uint32_t u = 0; u < 4u; ++u) {
            if (nib[u] == 15u) continue;
            const size_t q = q0 + 64u * u;
            uint8_t* g = p.grid + q * 16u;
            if (nib[u] == 0u) __builtin_nontemporal_store(z, reinterpret_cast<Zero4*>(g));
            else {
                // (a piece on the queued region's rim: plain stores -- four bytes that leave non-temporally reach the fabric as a partial write)
#pragma unroll
                for (uint32_t b = 0; b < 4u; ++b)
                    if (!((nib[u] >> b) & 1u)) *reinterpret_cast<uint32_t*>(g + 4u * b) = 0u;
            }
        }
        if (p.texels) {
            // the same bricks of the texel image: a piece is 64 bytes there.  Lane l of round k writes the (64 k + l)-th 16 bytes of the
            // wave's 4 KiB (consecutive lanes, consecutive bytes: a lane writing its own piece's four quarters would leave every store
            // instruction a quarter of each line) -- brick l & 3 of piece 16 k + (l >> 2), whose nibble lane 16 k + (l >> 2) holds
            const uint32_t lane = threadIdx.x;
#pragma unroll
            for (uint32_t u = 0; u < 4u; ++u) {
                uint32_t* t = p.texels + ((size_t)base + 64u * u) * 16u;
#pragma unroll
                for (uint32_t k = 0; k < 4u; ++k) {
                    const uint32_t n = (uint32_t)__shfl((int)nib[u], (int)(16u * k + (lane >> 2)));
                    if (!((n >> (lane & 3u)) & 1u)) __builtin_nontemporal_store(z, reinterpret_cast<Zero4*>(t + (64u * k + lane) * 4u));
                }
            }
        }
    }
}

// (the body; STARTS as in queue_bricks)
template <bool TEXELS, bool STARTS>
__device__ __forceinline__ void listed_brick(const VoxelizeParams& p, const QueueLens& lens, const ClearShare& clr)
{
#if defined(__HIP_DEVICE_COMPILE__)
    __shared__ int32_t stack[(TEXELS ? 20 : 16) * 64];     // per lane: 8 queued triangles of two words (TEXELS: then the closest hit's V, W, det, index)
    // The kernel's arguments, ALL asked for here: left to itself the compiler loads each word where it is first used, and the start of a
    // brick is then a chain of scalar-memory round trips each waited for before the next is asked for (the clear's share -> the sixteen
    // queue lengths -> the queue's address -> [the brick's word] -> the scene's words in two more batches).  Named here they are one batch of
    // loads behind one wait; only the brick's word itself is a second trip (-0.5 % on the full grid, -0.7 % on a rank's share).
    asm volatile("" :: "s"(lens.len[0]), "s"(lens.len[1]), "s"(lens.len[2]), "s"(lens.len[3]), "s"(lens.len[4]), "s"(lens.len[5]), "s"(lens.len[6]), "s"(lens.len[7]),
                 "s"(lens.heavy[0]), "s"(lens.heavy[1]), "s"(lens.heavy[2]), "s"(lens.heavy[3]), "s"(lens.heavy[4]), "s"(lens.heavy[5]), "s"(lens.heavy[6]),
                 "s"(lens.heavy[7]), "s"(clr.blocks), "s"(clr.where), "s"(clr.live), "s"(gridDim.x), "s"(p.queueSlots), "s"(p.queueCap));
    asm volatile("" :: "s"(p.N), "s"(p.z0), "s"(p.nz), "s"(p.zBlock), "s"(p.zPeriod), "s"(p.zShift), "s"(STARTS ? p.scene.dmStartCells : p.scene.dmCells), "s"(p.scene.dmEntries), "s"(p.scene.dmR),
                 "s"(p.scene.dmCoop), "s"(STARTS ? p.scene.dmStartCells : static_cast<const void*>(p.scene.dmStarts)), "s"(p.scene.triPos), "s"(p.grid), "s"(p.scene.rootLo[0]), "s"(p.scene.rootLo[1]), "s"(p.scene.rootLo[2]),
                 "s"(p.scene.rootHi[0]), "s"(p.scene.rootHi[1]), "s"(p.scene.rootHi[2]));
    uint32_t wg = blockIdx.x;
    if (clr.blocks) {
        // (clr.blocks is a multiple of 8: a brick workgroup's number keeps its residue mod 8 -- its XCD, its queue)
        const uint32_t bricks = gridDim.x - clr.blocks;
        if (clr.where == 3u) {
            // rows of 8 workgroups; of the launch's R rows C clear, spread evenly: row r clears iff floor((r + 1) C / R) > floor(r C / R),
            // and floor(r C / R) clearing rows lie in front of it -- the zeros leave as a trickle beside the bricks' loads, not as a burst
            const uint32_t r = wg >> 3, R = gridDim.x >> 3, C = clr.blocks >> 3;
            const uint32_t before = (uint32_t)(((uint64_t)r * C) / R), upto = (uint32_t)(((uint64_t)(r + 1u) * C) / R);
            if (upto != before) { clear_dead_bricks(p, clr.live, 8u * before + (wg & 7u), clr.blocks); return; }
            wg -= 8u * before;
        } else {
            const bool clears = clr.where == 1u ? wg < clr.blocks : wg >= bricks;
            if (clears) { clear_dead_bricks(p, clr.live, clr.where == 1u ? wg : wg - bricks, clr.blocks); return; }
            if (clr.where == 1u) wg -= clr.blocks;
        }
    }
    const uint32_t x = wg & 7u, k = wg >> 3;
#if defined(DXV_PHASE_TIMES)
    const unsigned long long tPhase0_ = __builtin_amdgcn_s_memrealtime();
#endif
#if defined(DXV_QUEUE_TIMES)
    const uint64_t tStart = __builtin_amdgcn_s_memrealtime();
    if (threadIdx.x == 0u && 3u * wg + 2u < p.redoCap) { p.redo[3u * wg] = 0; p.redo[3u * wg + 1u] = 0; }
#endif
    // (x's equal share of the launch: its own queue's first bricks, then what longer queues hold beyond theirs -- queue_item)
    uint32_t qy, qslot;
    if (!queue_item(lens, p.queueCap, x, k, qy, qslot)) return;
    // the brick's word through the SCALAR cache (one word per wave; the queue was written long before this launch): as a vector load it was
    // a round trip through the busy vector-memory pipe (~1 us of a 10 us brick) in front of everything else the workgroup does
    uint32_t w;
    {
        const uint32_t* slot = p.queueSlots + (uint32_t)__builtin_amdgcn_readfirstlane((int)(qy * p.queueCap + qslot));     // (8 cap <= 2^27 bricks)
        asm volatile("s_load_dword %0, %1, 0x0\n\ts_waitcnt lgkmcnt(0)" : "=s"(w) : "s"(slot) : "memory");
    }
    const SceneView& sc = p.scene;
    // (the brick's set-up, down to origin_leaves_root: the same sequence as in k_voxelize_queue, see there)
    const uint32_t N = p.N, nz = p.nz;
    const uint32_t bx = w & 1023u, by = (w >> 10) & 1023u, bz = w >> 20;
    const uint32_t tid = threadIdx.x;
    uint32_t ix, iy, lz;
    brick_voxel_clamped(N, nz, bx, by, bz, tid, ix, iy, lz);
    const uint32_t iz = global_slice(p.z0, nz, p.zBlock, p.zShift, p.zPeriod, lz);
    Ray r;
    ray_origin(N, ix, iy, iz, r.ox, r.oy, r.oz);
    const DirMapView dm{static_cast<const DirCell*>(sc.dmCells), static_cast<const DirEntry*>(sc.dmEntries), sc.dmR, sc.dmCoop, sc.dmStarts, static_cast<const DirCell*>(STARTS ? sc.dmStartCells : nullptr)};
    DirRayStart start = dm_ray_start<STARTS ? 2 : 0>(r.ox, r.oy, r.oz, dm);
    if (origin_leaves_root(r.ox, r.oy, r.oz, sc.rootLo, sc.rootHi)) start.live = false;
    Hit best;
    float bestDet = 1.0f;
    const StridedStack stk{stack + tid, 64};
#if defined(DXV_PHASE_TIMES)
    { const unsigned long long now_ = __builtin_amdgcn_s_memrealtime(); if (threadIdx.x == 0u) { unsigned long long* slot_ = g_dxvPhase + (size_t)(blockIdx.x & (kPhaseSlots - 1u)) * 16u; atomicAdd(slot_, now_ - tPhase0_); atomicAdd(slot_ + 6, 1ull); } }
#endif
    // (with the texel image on, the closest hit's V, W, det and index wait in the LDS column: four registers that cost that variant its
    // seventh wave per SIMD; without it the allocator does better with them in registers: 68 against 74)
    trace_reference_dm_from<StridedStack, 0, TEXELS ? 1 : 2, STARTS ? 2 : 0>(r, dm, start, sc.triPos, stk, 16, best, bestDet);
#if defined(DXV_PHASE_TIMES)
    const unsigned long long tPhase5_ = __builtin_amdgcn_s_memrealtime();
#endif
    uint32_t texel = 0;
    const uint8_t occ = TEXELS ? shade_reference_lds(sc, r, best.leaf, stk, 16, &texel) : shade_reference_again(sc, r, best.leaf);
    // the lane's voxel once more (nothing of it is kept through the body: with the texel image on, the lane's coordinates held across the
    // scan cost the kernel its seventh wave per SIMD -- k_voxelize_queue does the same)
    const uint32_t lane = lane_id();
    store_brick<TEXELS>(&p, N, nz, bx, by, bz, lane, occ, texel);
#if defined(DXV_PHASE_TIMES)
    { const unsigned long long now_ = __builtin_amdgcn_s_memrealtime(); if (threadIdx.x == 0u) atomicAdd(g_dxvPhase + (size_t)(blockIdx.x & (kPhaseSlots - 1u)) * 16u + 5, now_ - tPhase5_); }
#endif
#if defined(DXV_QUEUE_TIMES)
    // (diagnostic build only, tools/wg_times.py: start and end of every workgroup in 100 MHz ticks, and the XCD it ran on)
    if (threadIdx.x == 0u && 3u * wg + 2u < p.redoCap) {
        uint32_t xcc;
        asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(xcc));
        p.redo[3u * wg] = tStart; p.redo[3u * wg + 1u] = (__builtin_amdgcn_s_memrealtime() & 0x0fffffffffffffffull) | ((uint64_t)(xcc & 15u) << 60);
        p.redo[3u * wg + 2u] = w;
    }
#endif
#else
    (void)p;
#endif
}
// ... as kernels, like the queue's
template <bool TEXELS> __global__ __launch_bounds__(64, 6) void k_voxelize_listed(VoxelizeParams p, QueueLens lens, ClearShare clr) { listed_brick<TEXELS, true>(p, lens, clr); }
template <bool TEXELS> __global__ __launch_bounds__(64, 6) void k_voxelize_listed_plain(VoxelizeParams p, QueueLens lens, ClearShare clr) { listed_brick<TEXELS, false>(p, lens, clr); }

// persistent waves the current device holds at once (occupancy of the kernel x compute units), a multiple of 8.
// An answer about (device, kernel): the context keeps it (ListsOccupancy, dxv_device.h), nothing here does.
static uint32_t queue_waves(bool texels)
{
    int dev = 0, cus = 0, perCu = 0;
    if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || cus <= 0) cus = 256;
    const hipError_t e = texels ? hipOccupancyMaxActiveBlocksPerMultiprocessor(&perCu, k_voxelize_queue<true>, 64, 0)
                                : hipOccupancyMaxActiveBlocksPerMultiprocessor(&perCu, k_voxelize_queue<false>, 64, 0);
    if (e != hipSuccess || perCu <= 0) { (void)hipGetLastError(); perCu = 24; }
    return ((uint32_t)cus * (uint32_t)perCu + 7u) & ~7u;
}

// Dynamic LDS a launch of k_voxelize_listed<false> asks for WITHOUT using it.  The kernel fits eight waves per SIMD (64 VGPRs, 4 KB of LDS per
// single-wave workgroup: 32 workgroups per CU); how many it should run depends on how a brick's rays fall on the lists' map.  Where they
// look into neighbouring texels (grid side >= 3/4 of the map's) the eighth wave is throughput: -9 % at 512^3, -12 % at 1024^3 against seven.
// Where a brick is spread over many texels (256^3 on the 512 map) it is more lines in flight per load and slower bricks: +7 %.  Such a
// launch is held at 28 workgroups per CU by LDS: the smallest pad that leaves so many, found once per value through the occupancy query
// (26 .. 30 measure the same: the hardware fills SIMDs evenly; profiles/r06/ab_listed_workgroups_per_cu.jsonl).  Option listedwaves overrides.
static int listed_pad_for(uint32_t want)                                // the pad in bytes, -1: none
{
    int found = -1, perCu = 0;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&perCu, k_voxelize_listed<false>, 64, 0) == hipSuccess && perCu > (int)want) {
        for (int pad = 64; pad <= 16384; pad += 64) {
            if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&perCu, k_voxelize_listed<false>, 64, (size_t)pad) != hipSuccess) break;
            if (perCu <= (int)want) { found = pad; break; }
        }
    }
    (void)hipGetLastError();
    return found;
}
// ... asked once per context and value (up to 257 queries, in the first launch that needs it)
static uint32_t listed_lds_pad(const VoxelizeParams& p, ListsOccupancy& occ)
{
    if (p.texels) return 0u;                                           // (that variant holds 72 VGPRs: seven waves by itself)
    const uint32_t want = p.listedWaves ? p.listedWaves : (4u * p.N >= 3u * p.scene.dmR ? 32u : 28u);
    if (want >= 32u) return 0u;
    int& pad = occ.listedPad[want < 8u ? 8u : want];
    if (pad == 0) pad = listed_pad_for(want);
    return pad > 0 ? (uint32_t)pad : 0u;
}

// one workgroup per queued brick (and the clearing ones): the kernel that reads the start cells when the launch has a table, else the plain one
static hipError_t launch_listed(const VoxelizeParams& p, const QueueLens& lens, const ClearShare& clr, uint32_t wgs, ListsOccupancy& occ, hipStream_t s)
{
    const bool starts = p.scene.dmStartCells != nullptr;
    if (p.texels) { if (starts) k_voxelize_listed<true><<<dim3(wgs), dim3(64), 0, s>>>(p, lens, clr); else k_voxelize_listed_plain<true><<<dim3(wgs), dim3(64), 0, s>>>(p, lens, clr); }
    else {
        const uint32_t pad = listed_lds_pad(p, occ);
        if (starts) k_voxelize_listed<false><<<dim3(wgs), dim3(64), pad, s>>>(p, lens, clr); else k_voxelize_listed_plain<false><<<dim3(wgs), dim3(64), pad, s>>>(p, lens, clr);
    }
    return hipGetLastError();
}

// the sixteen count words of a queue as the host read them (eight lengths, of which heavy) -> kernel argument; returns
// listedLen = ceil(total / 8): the items of an XCD's equal share (queue_item)
static uint32_t queue_lens_from(const uint32_t lens16[16], QueueLens& lens)
{
    uint32_t total = 0;
    for (int a = 0; a < 8; ++a) { lens.len[a] = lens16[a]; lens.heavy[a] = lens16[8 + a]; total += lens16[a]; }
    return (total + 7u) / 8u;
}

// rebuild: clear the grid and build the queue in front of the launch (a launch that may not rely on anything an earlier
// launch left behind); else the caller vouches that the frame's grid and queue are those of the same launch made before
// (same lists, partition and buffers: the kernel writes the same bricks every time) and only the queue heads are reset.
hipError_t launch_voxelize_queue(const VoxelizeParams& p, ListsOccupancy& occ, bool rebuild, uint32_t* wavesOut, hipEvent_t* planEvents, const uint32_t* listedLens, hipStream_t s)
{
    QueueLens lens{};
    const uint32_t listedLen = listedLens ? queue_lens_from(listedLens, lens) : 0u;
    hipError_t e;
    if (!rebuild && listedLen) {
        // the queue as it stands, one workgroup per item of an XCD's equal share (listedLen = ceil(total / 8)) and per XCD
        if (wavesOut) *wavesOut = 8u * listedLen;
        return launch_listed(p, lens, ClearShare{nullptr, 0u, 0u}, 8u * listedLen, occ, s);
    }
    if (rebuild) {
        if (!p.planClear) {
            if ((e = hipMemsetAsync(p.grid, 0, (size_t)p.N * p.N * p.nz, s)) != hipSuccess) return e;
            if (p.texels && (e = hipMemsetAsync(p.texels, 0, (size_t)p.N * p.N * p.nz * 4, s)) != hipSuccess) return e;
        }
        if (planEvents && (e = hipEventRecord(planEvents[0], s)) != hipSuccess) return e;
        if ((e = plan_build(p, s)) != hipSuccess) return e;
        if (planEvents && (e = hipEventRecord(planEvents[1], s)) != hipSuccess) return e;
    } else if ((e = hipMemsetAsync(p.queue + queue_head_word(0, 0), 0, sizeof(uint32_t) * (queue_len_word(0) - queue_head_word(0, 0)), s)) != hipSuccess) return e;   // the 64 heads
    uint32_t& held = occ.queueWaves[p.texels ? 1 : 0];
    if (!held) held = queue_waves(p.texels != nullptr);
    const uint32_t sevenths = p.queueSevenths && p.queueSevenths < 7u ? p.queueSevenths : 7u;
    const uint32_t waves = p.queueWaves ? (p.queueWaves + 7u) & ~7u : (held * sevenths / 7u + 7u) & ~7u;     // (a multiple of 8, at least 8: every head has a home wave)
    if (wavesOut) *wavesOut = waves;
    const bool starts = p.scene.dmStartCells != nullptr;
    if (p.texels) { if (starts) k_voxelize_queue<true><<<dim3(waves), dim3(64), 0, s>>>(p); else k_voxelize_queue_plain<true><<<dim3(waves), dim3(64), 0, s>>>(p); }
    else { if (starts) k_voxelize_queue<false><<<dim3(waves), dim3(64), 0, s>>>(p); else k_voxelize_queue_plain<false><<<dim3(waves), dim3(64), 0, s>>>(p); }
    return hipGetLastError();
}

#if defined(DXV_PHASE_TIMES)
// diagnostic build: the phase sums of the lists kernel (dxv_dirmap.h, DXV_PHASE) since the last reset.  g_dxvPhase is per translation
// unit: this reads the copy of the two brick kernels of this file (k_voxelize<..., WALK 4> in traverse.hip has its own, which no tool reads)
hipError_t phase_times_read(unsigned long long out[16], bool reset)
{
    std::vector<unsigned long long> all((size_t)kPhaseSlots * 16u);
    hipError_t e = hipMemcpyFromSymbol(all.data(), HIP_SYMBOL(g_dxvPhase), all.size() * sizeof(unsigned long long));
    for (int k = 0; k < 16; ++k) out[k] = 0;
    for (size_t i = 0; i < all.size(); ++i) out[i & 15u] += all[i];
    if (e == hipSuccess && reset) {
        std::fill(all.begin(), all.end(), 0ull);
        e = hipMemcpyToSymbol(HIP_SYMBOL(g_dxvPhase), all.data(), all.size() * sizeof(unsigned long long));
    }
    return e;
}
#endif

// A launch through a PREPARED queue (dxv_device.h): the queue is a pure function of (static scene's lists, grid, partition) and was
// built when those were fixed -- Init, dxv_prepare_launch -- like the lists themselves (the reference builds everything its frames
// trace through once, Content/Voxelizer.cpp:73, and a frame is one DispatchRays, :351-369).  The launch clears the grid and runs every
// queued brick: every voxel is written in every launch, nothing a launch reads was left behind by another LAUNCH.
hipError_t launch_voxelize_prepared(const VoxelizeParams& p, ListsOccupancy& occ, const uint32_t lens16[16], const uint32_t* live, int clearMode, uint32_t* wavesOut, hipStream_t s)
{
    QueueLens lens{};
    const uint32_t listedLen = queue_lens_from(lens16, lens);
    if (wavesOut) *wavesOut = 8u * listedLen;
    const size_t bytes = (size_t)p.N * p.N * p.nz;
    ClearShare clr{nullptr, 0u, 0u};
    if (clearMode != 0 && live && (p.N & 15u) == 0u && listedLen) {
        // 1,024 sixteen-byte pieces per clearing workgroup (16 per thread)
        const uint64_t pieces = bytes >> 4;
        uint64_t blocks = ((pieces + 1023u) >> 10);
        blocks = (blocks + 7u) & ~(uint64_t)7u;
        clr.live = live; clr.blocks = (uint32_t)blocks; clr.where = (uint32_t)clearMode;
    } else {
        const hipError_t e = plan_clear_grid(p, s);                     // (a kernel of its own in front of the bricks': plan_bricks.hip)
        if (e != hipSuccess || !listedLen) return e;
    }
    const uint32_t wgs = 8u * listedLen + clr.blocks;
    return launch_listed(p, lens, clr, wgs, occ, s);
}

} // namespace dxv
