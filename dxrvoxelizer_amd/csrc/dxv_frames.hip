// dxv_frames.hip -- frames, launches and work queues: what a dxv_voxelize* call puts into a frame's stream (launch_now), what
// dxv_sync reads back (sync_frame), and the C-ABI entry points around them.  Whether a launch builds its queue, keeps it or has
// the hardware deal it out is dxv_policy.h's queue_policy.
#include "dxv_ctx.h"

using namespace dxv;
using namespace dxvhost;

namespace dxvhost {

// status words, redo list, events and (frames 1..) the stream of a frame, on its first use
int frame_prepare(dxv_ctx* c, uint32_t i)
{
    Frame& f = c->frames[i];
    if (f.ready) return 0;
    if (i && !f.ownStream) DXV_HIP(c, hipStreamCreateWithFlags(&f.ownStream, hipStreamNonBlocking));
    for (Timer& t : f.timers) {
        if (!t.e0) DXV_HIP(c, hipEventCreate(&t.e0));
        if (!t.e1) DXV_HIP(c, hipEventCreate(&t.e1));
    }
    if (!f.evEnd) DXV_HIP(c, hipEventCreateWithFlags(&f.evEnd, hipEventDisableTiming));
    DXV_HIP(c, f.status.reserve(64, 256));
    DXV_HIP(c, f.redo.reserve(kRedoCap, sizeof(uint64_t) * kRedoCap));
    // on the frame's own stream, and finished before anything reads the words: the streams are non-blocking, a memset on the
    // null stream is not ordered with them (a fresh context whose status words landed on recycled memory could read
    // 0x7ff out of them -- seen twice in some fifty runs of the GPU suite)
    DXV_HIP(c, hipMemsetAsync(f.status.p, 0, 256, frame_stream(c, i)));
    DXV_HIP(c, hipStreamSynchronize(frame_stream(c, i)));
    f.ready = true;
    return 0;
}

// ---------------------------------------------------------------------------------------------
// Prepared work queues (include/dxv.h: dxv_prepare_launch).  A slot is valid while its epoch is the lists' epoch; everything
// that changes the scene calls drop_prepared as well (a refit keeps the epoch until the lists are rebuilt).
// ---------------------------------------------------------------------------------------------
void drop_prepared(dxv_ctx* c)
{
    for (auto& q : c->prepared) { q.epoch = 0; q.bricks = 0; }
}
// the sixteen count words of a queue header as the device wrote them (from queue_len_word(0) on, each in a line of its own) ->
// the eight lengths and how many of each are heavy; returns the bricks queued
static uint32_t decode_queue_lens(const uint32_t* words, uint32_t lens[16])
{
    uint32_t bricks = 0;
    for (uint32_t x = 0; x < 8u; ++x) {
        lens[8u + x] = words[queue_heavy_word(x) - queue_len_word(0)];
        lens[x] = words[queue_len_word(x) - queue_len_word(0)] + lens[8u + x];
        bricks += lens[x];
    }
    return bricks;
}
int check_grid(dxv_ctx* c, const char* who, uint32_t N, bool orZero)
{
    if (orZero && !N) return 0;
    if (N < 2 || (N & 1u) || N > 2048) return fail(c, "%s: grid_dim must be %seven and in [2, 2048], got %u", who, orZero ? "0 or " : "", N);
    return 0;
}
int check_slab(dxv_ctx* c, const char* who, uint32_t N, uint32_t z0, uint32_t nz)
{
    if (check_grid(c, who, N)) return 1;
    if (nz == 0 || z0 >= N || nz > N - z0) return fail(c, "%s: slab [%u, %u+%u) outside the grid (N=%u)", who, z0, z0, nz, N);
    return 0;
}
int check_interleave(dxv_ctx* c, const char* who, uint32_t N, uint32_t rank, uint32_t world, uint32_t zblock)
{
    if (!world || rank >= world || !zblock || (zblock & (zblock - 1u)) || N % (zblock * world))
        return fail(c, "%s: need rank < world, zblock a power of two and grid_dim %% (zblock * world) == 0 "
                       "(N=%u, world=%u, zblock=%u)", who, N, world, zblock);
    return 0;
}
static uint32_t queue_region_bits(const dxv_ctx* c, uint32_t N, uint32_t nz) { return c->opt.planregion ? (uint32_t)c->opt.planregion : plan_region_bits(N, nz); }
static int find_prepared(const dxv_ctx* c, uint32_t N, uint32_t z0, uint32_t nz, uint32_t zBlock, uint32_t zPeriod)
{
    if (!c->listEpoch || c->lists.state != 1) return -1;
    const uint32_t rb = queue_region_bits(c, N, nz);
    for (uint32_t i = 0; i < dxv_ctx::kPreparedSlots; ++i) {
        const auto& q = c->prepared[i];
        if (q.epoch == c->listEpoch && q.N == N && q.z0 == z0 && q.nz == nz && q.zBlock == zBlock && q.zPeriod == zPeriod && q.regionBits == rb &&
            q.planHeavy == (uint32_t)c->opt.planheavy && q.mem.p)
            return (int)i;
    }
    return -1;
}
// slices: local lz in [0, nzLocal) <-> global z0 + (lz / zBlock) * zPeriod + lz % zBlock (as voxelize_common)
static int prepare_partition(dxv_ctx* c, uint32_t N, uint32_t z0, uint32_t nzLocal, uint32_t zBlock, uint32_t zPeriod)
{
    if (!c->haveScene) return fail(c, "dxv_prepare_launch: no scene (call dxv_build or dxv_scene_import first)");
    DXV_HIP(c, hipSetDevice(c->device));
    c->prepareMs = 0.0f;
    if (!c->opt.lists || !c->opt.plan || c->opt.brick != 4 || c->opt.ablate) return 0;     // (launches of this context do not go through a queue)
    if (settle_lists(c)) return 1;
    if (c->lists.state == 0 || c->lists.opt != c->opt.listres) {
        if (dxv_build_lists_for_grid(c, 0)) return 1;
    }
    if (c->lists.state != 1 || !c->lists.mip.p) return 0;                       // a scene without lists (over the caps): tree walks, nothing to prepare
    if (find_prepared(c, N, z0, nzLocal, zBlock, zPeriod) >= 0) return 0;
    if (sync_frames(c)) return 1;                                      // (a slot that is reused may still be read by a launch in flight)
    // a slot: one whose key is this partition's (stale epoch), else a free one, else the least recently used
    int slot = -1;
    for (uint32_t i = 0; i < dxv_ctx::kPreparedSlots && slot < 0; ++i) {
        const auto& q = c->prepared[i];
        if (q.mem.p && q.N == N && q.z0 == z0 && q.nz == nzLocal && q.zBlock == zBlock && q.zPeriod == zPeriod) slot = (int)i;
    }
    for (uint32_t i = 0; i < dxv_ctx::kPreparedSlots && slot < 0; ++i)
        if (c->prepared[i].epoch != c->listEpoch) slot = (int)i;
    if (slot < 0) {
        slot = 0;
        for (uint32_t i = 1; i < dxv_ctx::kPreparedSlots; ++i)
            if (c->prepared[i].used < c->prepared[slot].used) slot = (int)i;
    }
    auto& q = c->prepared[slot];
    q.epoch = 0; q.bricks = 0;
    uint32_t cap = 0;
    const size_t words = kQueueHeaderWords + (plan_queue_words(N, nzLocal, &cap) - kQueueSlotsAt), liveWords = plan_live_words(N, nzLocal);
    DXV_HIP(c, q.mem.reserve(words, sizeof(uint32_t) * words));
    DXV_HIP(c, q.live.reserve(liveWords, sizeof(uint32_t) * liveWords));
    const hipStream_t s = c->stream;
    VoxelizeParams p{};
    scene_params(c, p.scene);
    lists_params(c, p.scene);
    p.N = N; p.z0 = z0; p.nz = nzLocal; p.zBlock = zBlock; p.zPeriod = zPeriod; p.zShift = z_shift(zBlock);
    p.queue = q.mem.p; p.queueSlots = q.mem.p + kQueueHeaderWords; p.queueCap = cap; p.mip = c->lists.mip.p;
    p.planRegionBits = queue_region_bits(c, N, nzLocal); p.planHeavy = (uint32_t)c->opt.planheavy;
    p.planClear = 0u; p.queueZero = nullptr; p.liveMask = q.live.p;
    DXV_HIP(c, hipEventRecord(c->ev[8], s));
    DXV_HIP(c, hipMemsetAsync(q.mem.p, 0, sizeof(uint32_t) * kQueueHeaderWords, s));
    DXV_HIP(c, hipMemsetAsync(q.live.p, 0, sizeof(uint32_t) * liveWords, s));
    DXV_HIP(c, plan_build(p, s));
    DXV_HIP(c, hipMemcpyAsync(c->pin->preparedLens, q.mem.p + queue_len_word(0), sizeof(c->pin->preparedLens), hipMemcpyDeviceToHost, s));
    DXV_HIP(c, hipStreamSynchronize(s));
    q.bricks = decode_queue_lens(c->pin->preparedLens, q.lens);
#if !defined(DXV_PREPARED_ORDER_MORTON)                                 // (scratch builds: the order as built, for an A/B)
    // A queue that is launched again and again is worth a sort: direction-major, whole map tiles dealt to the XCDs (queue_order.hip).
    // The same bricks in another order: the live mask stands.  Two more host round trips of an Init, for the number of keys and for
    // the new counts -- the deal knows nothing of a queue's capacity, so a queue that is given more than it holds gets more memory.
    DevBuf<uint8_t> orderOnce;
    if (q.bricks) {
        // (the sort's scratch: the list build's key buffers where the context still has them -- the build is over, settle_lists above --
        // else an allocation of this call's own, ~0.1 ms inside prepare_ms)
        const size_t scratchBytes = queue_order_scratch_bytes(q.bricks);
        uint8_t* orderScratch = c->listScratchB.p;
        if (c->listScratchB.cap < scratchBytes) {
            DXV_HIP(c, orderOnce.reserve(scratchBytes, scratchBytes));
            orderScratch = orderOnce.p;
        }
        const uint64_t* sorted = nullptr;
        const uint32_t* counts = nullptr;
        DXV_HIP(c, queue_order_sort(p, q.lens, q.bricks, orderScratch, &sorted, &counts, s));
        DXV_HIP(c, hipMemcpyAsync(c->pin->preparedLens, counts, 16 * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
        DXV_HIP(c, hipStreamSynchronize(s));
        uint32_t longest = 0;
        for (uint32_t x = 0; x < 8u; ++x) {
            q.lens[8u + x] = c->pin->preparedLens[x];
            q.lens[x] = c->pin->preparedLens[x] + c->pin->preparedLens[8u + x];
            longest = q.lens[x] > longest ? q.lens[x] : longest;
        }
        if (longest > cap) {
            cap = (longest + 63u) & ~63u;
            const size_t grown = kQueueHeaderWords + 8u * (size_t)cap;
            DXV_HIP(c, q.mem.reserve(grown, sizeof(uint32_t) * grown));
            p.queue = q.mem.p; p.queueSlots = q.mem.p + kQueueHeaderWords; p.queueCap = cap;
        }
        DXV_HIP(c, hipMemsetAsync(q.mem.p, 0, sizeof(uint32_t) * kQueueHeaderWords, s));
        DXV_HIP(c, queue_order_write(p, q.lens, q.bricks, sorted, s));
    }
#endif
    DXV_HIP(c, hipEventRecord(c->ev[9], s));
    DXV_HIP(c, hipStreamSynchronize(s));
    q.N = N; q.z0 = z0; q.nz = nzLocal; q.zBlock = zBlock; q.zPeriod = zPeriod; q.regionBits = p.planRegionBits; q.planHeavy = p.planHeavy; q.cap = cap;
    q.ms = elapsed(c->ev[8], c->ev[9]);
    q.used = ++c->preparedClock;
    q.epoch = c->listEpoch;
    c->prepareMs = q.ms;
    c->stats.prepare_ms = q.ms;
    return 0;
}

// the far-radius map of the current scene (a scene without lists), on the frame's stream and finished before any other stream can use it
int ensure_far_map(dxv_ctx* c, hipStream_t s)
{
    FarMap& m = c->farMap;
    if (m.epoch == c->sceneEpoch && m.mip.p) return 0;
    // (coarse: a 4^3-voxel brick of a 512^3 grid is a texel of the 128 map wide where the map is finest; the test reads a max-mip level
    // that holds the brick's patch in 2 x 2 cells anyway)
    const uint32_t R = c->hdr.numTris < 20000u ? 64u : 128u;
    DXV_HIP(c, m.far32.reserve(R, sizeof(uint32_t) * 6u * R * R));
    DXV_HIP(c, m.cells.reserve(R, sizeof(DirCell) * 6u * R * R));
    DXV_HIP(c, m.mip.reserve(R, sizeof(uint16_t) * (size_t)dm_mip_buffer_words(R)));
    m.epoch = 0;
    DXV_HIP(c, hipEventRecord(c->ev[8], s));
    DXV_HIP(c, dirmap_far(scene_tripos(c), c->hdr.numTris, R, m.far32.p, m.cells.p, m.mip.p, s));
    DXV_HIP(c, hipEventRecord(c->ev[9], s));
    DXV_HIP(c, hipStreamSynchronize(s));
    m.ms = elapsed(c->ev[8], c->ev[9]);
    m.R = R;
    m.epoch = c->sceneEpoch;
    return 0;
}

// Everything that changes what the frames read (mesh, scene, lists, options that rebuild) first lets every
// frame finish -- including the status check and, if a launch asked for it, the relaunch against the OLD scene.
int sync_frames(dxv_ctx* c)
{
    for (uint32_t i = 0; i < DXV_FRAME_COUNT; ++i)
        if (c->frames[i].ready && sync_frame(c, i)) return 1;
    return settle_lists(c);
}

// Stack policy.  The stack never needs more than treeHeight entries, but rays rarely push more
// than a dozen, and LDS (entries * 4 B * threads) is what limits resident waves.  Launches use 20
// entries; the few rays that run out of them are listed and finished by k_voxelize_redo with a
// 64-entry column right behind the launch.  Only when a launch fills that list does it report
// through the status word, and dxv_sync then re-runs it with the next larger depth (up to the
// always-sufficient one) and keeps that depth for this scene.
// (+3: the postponed-leaf traversal keeps room for one push and two queued leaves)
// The wide walk pushes up to three entries per wide level (two binary levels) and keeps room for
// four more slots: 3 * ceil(h / 2) + 5.  Trees too deep for the largest column use the binary walk.
bool use_wide(const dxv_ctx* c, int mode)
{
    const int need = 3 * (((int)c->hdr.treeHeight + 1) / 2) + 5;
    return mode == DXV_MODE_REFERENCE && c->opt.wide && c->hdr.hasWide && c->opt.queue && need <= 64;
}
int safe_stack(const dxv_ctx* c, int mode)
{
    if (use_wide(c, mode)) return stack_round_up(3 * (((int)c->hdr.treeHeight + 1) / 2) + 5);
    return stack_round_up((int)c->hdr.treeHeight + 3);
}

// The surface pass of the frame's partition (surface.hip), on the frame's stream behind whatever is in it: sets the voxels the surface
// rule accepts, writes nothing else.  Reads the triangle records alone: no lists, no tree, no queue.
static int enqueue_surface(dxv_ctx* c, uint32_t frame, hipStream_t fs)
{
    Frame& f = c->frames[frame];
    const size_t bytes = surface_scratch_bytes(c->hdr.numTris);
    DXV_HIP(c, f.surf.reserve(bytes, bytes, fs));                       // (only this frame's stream uses it)
    SurfaceParams sp{};
    sp.triPos = scene_tripos(c); sp.T = c->hdr.numTris;
    sp.grid = f.grid.p; sp.N = f.grid_dim; sp.z0 = f.z0; sp.nz = f.nz; sp.zBlock = f.lastZBlock; sp.zPeriod = f.lastZPeriod;
    sp.scratch = f.surf.p; sp.items = (uint32_t)c->opt.surfaceitems;
    DXV_HIP(c, launch_surface(sp, fs));
    return 0;
}

// ---------------------------------------------------------------------------------------------
// A launch (launch_now, at the end) is the sequence of the stages below; what one stage decides and a later one needs is here.
// ---------------------------------------------------------------------------------------------
struct Launch {
    dxv_ctx* c;
    Frame& f;
    hipStream_t fs;
    bool relaunch;
    VoxelizeParams p;
    uint64_t voxels;
    int stack;                       // column depth of a tree walk
    bool queued;                     // the launch goes through a work queue ...
    int prep;                        // ... the context's prepared one of this slot (-1: the frame's own)
    int clear_for_surface();
    int apply_lists_step(bool& use);
    int attach_lists();
    int choose_queue();
    int attach_row_lists();
    int attach_far_map();
    int dispatch_rows();
    int dispatch_queue();
    int dispatch_bricks();
};

static ListsState lists_state(const dxv_ctx* c)
{
    ListsState s{};
    s.optLists = c->opt.lists; s.optListRes = c->opt.listres; s.listOpt = c->lists.opt; s.listState = c->lists.state; s.listRes = c->lists.res;
    s.listEntries = c->lists.count; s.numTris = c->hdr.numTris; s.launchesOfScene = c->launchesOfScene; s.refitted = c->refitted;
    s.floorTried = c->listFloorTried;
    return s;
}

// The surface rule alone (mode 2): outside the lists' policy (no build, no launch count, no queue, no far map, no tree), nothing to
// report afterwards; the partition is cleared here and the scatter of the launch's tail sets its voxels.
int Launch::clear_for_surface()
{
    f.plan_bricks = 0; f.plan_waves = 0; f.plan_ms = 0.0f;
    f.lastQueued = false; f.lastPrepared = -1; f.lastRedoParity = -1; f.lastCanFail = false;
    f.stack_entries = 0;
    if (c->opt.events) DXV_HIP(c, hipEventRecord(f.timers[kTimerLaunch].e0, fs));
    DXV_HIP(c, hipMemsetAsync(f.grid.p, 0, f.gridBytes, fs));
    return 0;
}

// WHEN the lists are built and on WHICH map is dxv_policy.h's lists_step (a pure function of lists_state: tests/test_policy.py
// walks its transitions): a first launch that is large enough may build them at once (lists = 1; the build's own estimate
// decides after its counting pass), a scene launched AGAIN without a refit in between is static and moves to the fine map, once;
// otherwise they are built when they are wanted and not there.  (A scene whose Init built them -- the host mirrors' -- meets none
// of this: its first launch is already the launch every later one is.)  Carries the step out; `use`: the launch goes through them.
int Launch::apply_lists_step(bool& use)
{
    ListsStep step = lists_step(lists_state(c), voxels, relaunch);
    if (step == ListsStep::build_if_it_pays) {
        if (sync_frames(c)) return 1;
        if (build_lists(c, fs, voxels, true)) return 1;             // (declined: the state stays 0, this launch walks the tree, the second one builds)
        step = lists_step(lists_state(c), 0, relaunch);               // (asked once per launch)
    }
    if (step == ListsStep::move_to_fine_map) {
        if (sync_frames(c)) return 1;
        c->listResFloor = kListsFineMap; c->listFloorTried = true;
        if (build_lists(c, fs)) return 1;
        step = lists_step(lists_state(c), 0, relaunch);
    }
    if (step == ListsStep::build && build_lists(c, fs, 0, true)) return 1;      // (this launch queues behind the build; its verdict: sync_frame)
    use = lists_used(lists_state(c), relaunch);                                 // (with the scene's launch count as it stood in front of this launch)
    if (!relaunch) ++c->launchesOfScene;
    return 0;
}

// the launch reads the lists: their fields of the parameters, and what the frame remembers about it
int Launch::attach_lists()
{
    // lists built on another frame's stream whose end nobody has waited for yet: this stream waits for it on the device
    if (c->listCheckPending && c->listCheckStream != fs) DXV_HIP(c, hipStreamWaitEvent(fs, c->evList[3], 0));
    f.usedLists = true; f.listEpochUsed = c->listEpoch;
    p.lists = 1u;
    p.ablate = (uint32_t)c->opt.ablate;
    lists_params(c, p.scene);
    p.scene.dmCoop = (uint32_t)c->opt.coop; p.listedWaves = (uint32_t)c->opt.listedwaves;
    stack = 16;                                                       // no stack: the column is the queue of selected triangles (8 items of two words)
    if (c->opt.region == 6) p.regionBits = 9u;                          // larger XCD regions suit the lists (-4 %); an explicit option wins
    f.list_entries = c->lists.count; f.list_res = c->lists.res;
    return 0;
}

// The work queue of a launch through the lists: one PREPARED for this very launch (dxv_prepare_launch, Init with a grid hint) --
// then the frame needs none of its own -- else the frame's own, sized for the partition (worst case: every brick live), else none.
int Launch::choose_queue()
{
    if (c->opt.brick != 4 || c->opt.ablate || !c->opt.plan || !c->lists.mip.p) return 0;
    prep = c->opt.prepared ? find_prepared(c, p.N, p.z0, p.nz, p.zBlock, p.zPeriod) : -1;
    uint32_t cap = 0;                                                   // words per XCD queue of this partition
    const size_t words = prep >= 0 ? 0 : plan_queue_words(p.N, p.nz, &cap);
    if (words > f.queue.cap) {
        const hipError_t qe = f.queue.reserve(words, sizeof(uint32_t) * words, fs);
        if (qe == hipSuccess) {
            DXV_HIP(c, hipMemsetAsync(f.queue.p, 0, sizeof(uint32_t) * kQueueSlotsAt, fs));      // both headers
            f.queueHdr = 0; f.queueOtherClear = true;
        }
        else if (qe == hipErrorOutOfMemory) (void)hipGetLastError();   // no queue: the brick-box launch still works
        else return fail(c, "work queue: hipMalloc failed: %s", hipGetErrorString(qe));
        f.clearSig = 0;
    }
    if (prep >= 0) {
        const auto& q = c->prepared[prep];
        queued = true; p.queue = q.mem.p; p.queueSlots = q.mem.p + kQueueHeaderWords; p.queueCap = q.cap;
        p.mip = c->lists.mip.p; p.planRegionBits = q.regionBits; p.planHeavy = q.planHeavy;
    }
    else if (f.queue.p) {
        queued = true; p.queue = f.queue.p + f.queueHdr * kQueueHeaderWords; p.queueSlots = f.queue.p + kQueueSlotsAt; p.queueCap = cap;
        p.mip = c->lists.mip.p; p.queueWaves = (uint32_t)c->opt.queuewaves; p.queueSevenths = queue_waves_sevenths(c->hdr.numTris, c->lists.res, p.N); p.queueHeads = (uint32_t)c->opt.queueheads; p.queueMinBricks = (uint32_t)c->opt.queuemin;
        p.planRegionBits = queue_region_bits(c, p.N, p.nz);
        p.planClear = c->opt.fuse ? 1u : 0u;
        p.planHeavy = (uint32_t)c->opt.planheavy;
    }
    return 0;
}

// parity rule: row lists from the scene's second parity launch on (their build, two passes of atomic additions per
// entry, costs 2 ms at 1 M triangles -- as much as three launches through the tree at 512^3, five with what the lists
// save: a mesh refitted every frame stays on the tree); plists = 2: from the first
// ... and only while triangles are small in voxels: a row's candidates are set up per row, and where a triangle spans
// many rows the 4 x 4 row blocks of the walk share that work (mean box extent in voxels, lists / walk in ms: torus-1M
// at 1024^3 1.7: 1.31 / 2.02; dragon x9 2.3: 1.26 / 1.49; dragon at 512^3 3.5: 0.16 / 0.36; bunny 5: 0.20 / 0.27;
// dragon at 1024^3 7: 1.18 / 0.88; bunny 10: 1.36 / 0.98)
int Launch::attach_row_lists()
{
    if (p.mode != DXV_MODE_PARITY || !c->opt.rows || c->opt.rowblock) return 0;
    const bool small = c->hdr.triExtent * 0.5f * (float)p.N <= 6.0f;
    const bool want = c->opt.plists && (relaunch ? c->rowLists.state == 1 : (c->opt.plists == 2 || (small && (c->parityLaunchesOfScene > 0 || c->rowLists.state != 0))));
    if (!relaunch) ++c->parityLaunchesOfScene;
    if (want && c->rowLists.state == 0) {
        if (sync_frames(c)) return 1;
        if (build_plists(c, fs)) return 1;
    }
    if (want && c->rowLists.state == 1) {
        p.scene.plCells = c->rowLists.cells.p; p.scene.plEntries = c->rowLists.entries.p; p.scene.plR = c->rowLists.res;
        f.list_entries = c->rowLists.count; f.list_res = c->rowLists.res;
    }
    return 0;
}

// a launch over the brick box (tree walk, or the lists under plan = 0): every workgroup makes the queue's brick test itself --
// against the lists' max-mip when the scene has (settled) lists, else against the far-radius map of the triangles' own
// footprints (dirmap_far: 0.13 ms at 1 M triangles), made at the scene's SECOND such launch -- a mesh refitted every frame
// goes without (dxv_policy.h, far_map_build_now)
int Launch::attach_far_map()
{
    if (p.mode != DXV_MODE_REFERENCE || queued || !c->opt.farmap || c->opt.brick != 4 || c->opt.ablate) return 0;
    if (c->boxLaunchEpoch != c->sceneEpoch) { c->boxLaunchEpoch = c->sceneEpoch; c->boxLaunchesOfScene = 0; }
    const bool haveFar = c->farMap.epoch == c->sceneEpoch && c->farMap.mip.p;
    if (c->lists.state == 1 && c->lists.mip.p && !c->listCheckPending) { p.mip = c->lists.mip.p; p.mipR = c->lists.res; }
    else if (haveFar || far_map_build_now(haveFar, c->boxLaunchesOfScene)) {
        if (ensure_far_map(c, fs)) return 1;
        p.mip = c->farMap.mip.p; p.mipR = c->farMap.R;
    }
    if (!relaunch) ++c->boxLaunchesOfScene;
    return 0;
}

// parity rule, one walk (or one row list) per grid row
int Launch::dispatch_rows()
{
    // rows whose triangles span several voxels share a walk: 4 x 4 rows per wave above 1.5 voxels of
    // mean triangle extent, 2 x 2 above 1.2 -- as long as the launch still has enough waves to fill
    // the GPU twice (blocks of a small grid or a thin slab leave it idle).  Measured crossovers:
    // profiles/r01/final/rowblock.jsonl; voxel-sized triangles are 1.2-2x slower in blocks, 4-7
    // voxel ones 3-5x faster.
    const float voxels = c->hdr.triExtent * 0.5f * (float)p.N;
    const uint64_t nseg = (p.N + 511u) / 512u;
    auto waves = [&](uint32_t rb) { return (uint64_t)((p.N + rb - 1u) / rb) * ((p.nz + rb - 1u) / rb) * nseg; };
    int rowBlock = 1;
    if (voxels > 1.5f && waves(4) >= 12288u) rowBlock = 4;
    else if (voxels > 1.2f && waves(2) >= 12288u) rowBlock = 2;
    if (c->opt.rowblock) rowBlock = c->opt.rowblock;
    if (p.scene.plCells) rowBlock = 1;                                 // row lists: one row per wave
    f.row_block = (uint32_t)rowBlock;
    f.clearSig = 0;                                                    // (the row kernel writes every voxel of the grid)
    DXV_HIP(c, launch_parity_rows(p, rowBlock, fs));
    f.lastRedoParity = -1;
    return 0;
}

// through a work queue: prepared, kept or built by this launch (dxv_policy.h: queue_policy)
int Launch::dispatch_queue()
{
    // The grid's zeros outside the queued bricks and the queue itself are still good when the frame's last writer was this
    // very launch -- same lists, partition and buffers (the kernel writes the same bricks every time): the frame's signature
    // word says so, every other writer of the grid resets it.  plan = 2, or a grid whose pointer the caller holds: never.
    uint64_t sig = 0;
    auto mix = [&](uint64_t v) { sig = (sig ^ v) * 0x9E3779B97F4A7C15ull; sig ^= sig >> 29; };
    mix(0x7175657565ull); mix(c->listEpoch); mix(p.N); mix(p.nz); mix(p.z0); mix(p.zBlock); mix(p.zPeriod);
    mix(reinterpret_cast<uint64_t>(p.grid)); mix(reinterpret_cast<uint64_t>(p.texels)); mix(reinterpret_cast<uint64_t>(f.queue.p));
    mix(p.planRegionBits); mix(p.planHeavy);
    sig |= 1ull;
    // (dxv_policy.h: every launch builds its queue under plan = 2; a kept queue whose lengths an earlier dxv_sync has read is
    // dealt out by the hardware -- option dispatch: 1 = whenever known, 2 = for partitions of up to 2^25 voxels)
    QueueState qs{};
    qs.optPlan = c->opt.plan; qs.optDispatch = c->opt.dispatch; qs.ptrExposed = f.ptrExposed; qs.keptSig = f.clearSig; qs.lensSig = f.queueLenSig;
    qs.queuedBricks = f.plan_bricks;
    qs.optPrepared = c->opt.prepared; qs.prepared = prep >= 0;
    const QueueLaunch how = queue_policy(qs, sig, voxels);
    if (how == QueueLaunch::prepared_hardware) {
        // queue from Init; the grid cleared and every queued brick written inside this launch; the frame keeps nothing
        auto& q = c->prepared[prep];
        q.used = ++c->preparedClock;
        f.clearSig = 0; f.queueLenSig = 0;
        DXV_HIP(c, launch_voxelize_prepared(p, c->occupancy, q.lens, q.live.p, c->opt.prepclear, &f.plan_waves, fs));
        f.plan_bricks = q.bricks; f.plan_ms = 0.0f;
        f.lastPrepared = prep;
        return 0;
    }
    const bool rebuild = how == QueueLaunch::build_and_persistent;
    hipEvent_t pe[2] = {f.timers[kTimerQueue].e0, f.timers[kTimerQueue].e1};
    const uint32_t* listed = how == QueueLaunch::kept_hardware ? f.queueLens : nullptr;
    if (rebuild) {
        // the new queue goes into the frame's other header, which the last build left cleared; this build clears the one it leaves
        const uint32_t target = f.queueHdr ^ 1u;
        p.queue = f.queue.p + target * kQueueHeaderWords;
        p.queueZero = f.queue.p + f.queueHdr * kQueueHeaderWords;
        if (!f.queueOtherClear) DXV_HIP(c, hipMemsetAsync(p.queue, 0, sizeof(uint32_t) * kQueueHeaderWords, fs));
        f.queueOtherClear = false;                                     // (until this launch is in the stream)
        f.clearSig = 0; f.queueLenSig = 0;
    }
    DXV_HIP(c, launch_voxelize_queue(p, c->occupancy, rebuild, &f.plan_waves, rebuild && c->opt.events ? pe : nullptr, listed, fs));
    if (rebuild) { f.queueHdr ^= 1u; f.queueOtherClear = true; }
    f.clearSig = f.ptrExposed ? 0 : sig;
    f.lastQueued = true; f.lastRebuilt = rebuild;
    return 0;
}

// the brick kernels (through a queue, or over the brick box), then the redo pass of the rays whose column ran out
int Launch::dispatch_bricks()
{
    if (queued) { if (dispatch_queue()) return 1; }
    else DXV_HIP(c, launch_voxelize(p, c->opt.brick, stack, fs));
    if (p.lists) f.lastRedoParity = -1;                              // no column to run out of, nothing to redo
    else {
        DXV_HIP(c, launch_voxelize_redo(p, fs));
        f.lastRedoParity = (int)f.redoParity;
        f.redoParity ^= 1u;
    }
    return 0;
}

// relaunch: the same launch again with a deeper column (sync_frame, after a walk reported an overflow) -- possibly on behalf of
// a caller that is about to replace the scene (sync_frames): it builds nothing, it takes the candidate structures that exist.
int launch_now(dxv_ctx* c, uint32_t frame, bool relaunch)
{
    Frame& f = c->frames[frame];
    Launch L{c, f, frame_stream(c, frame), relaunch, VoxelizeParams{}, 0, c->opt.stack ? c->opt.stack : c->stackNow, false, -1};
    const hipStream_t fs = L.fs;
    VoxelizeParams& p = L.p;
    scene_params(c, p.scene);
    p.grid = f.grid.p; p.texels = c->texels ? f.texels.p : nullptr; p.status = f.status.p;
    p.clearSig = &f.clearSig;
    p.redo = f.redo.p; p.redoCap = kRedoCap; p.redoParity = f.redoParity;
    p.N = f.grid_dim; p.z0 = f.z0; p.nz = f.nz; p.mode = ray_rule(f.lastMode);
    p.zBlock = f.lastZBlock; p.zPeriod = f.lastZPeriod; p.zShift = z_shift(p.zBlock);
    p.morton = (uint32_t)c->opt.morton;
    p.regionBits = (uint32_t)c->opt.region;
    p.queued = (uint32_t)c->opt.queue;
    p.subbox = (uint32_t)c->opt.subbox;
    p.wide = use_wide(c, p.mode) ? (uint32_t)c->opt.wide : 0u;      // 1: four-box nodes, 2: on wave-uniform visits only
    L.voxels = (uint64_t)p.N * p.N * p.nz;
    f.list_entries = 0; f.list_res = 0;
    f.usedLists = false;
    if (f.lastMode == DXV_MODE_SURFACE) {
        if (L.clear_for_surface()) return 1;
    } else {
        bool useLists = false;
        if (p.mode == DXV_MODE_REFERENCE && L.apply_lists_step(useLists)) return 1;
        if (useLists && (L.attach_lists() || L.choose_queue())) return 1;
        if (!L.queued) { f.plan_bricks = 0; f.plan_waves = 0; f.plan_ms = 0.0f; }
        f.lastQueued = false; f.lastPrepared = -1;
        if (f.ptrExposed) p.clearSig = nullptr;                            // the caller may have written into the grid: clear it every time
        L.stack = stack_for_brick(c->opt.brick, L.stack);                  // (shapes other than the shipped one are compiled for three depths)
        f.stack_entries = (uint32_t)L.stack;
        f.lastCanFail = true;
        if (L.attach_row_lists()) return 1;
        if (!p.lists && !p.scene.plCells && ensure_nodes(c, fs)) return 1;  // a tree walk after a refit: its copies of the hierarchy first
        if (L.attach_far_map()) return 1;
        const bool rows = p.mode == DXV_MODE_PARITY && c->opt.rows;
        f.lastCanFail = !((p.mode == DXV_MODE_REFERENCE && p.lists) || (rows && p.scene.plCells));
        if (c->opt.events) DXV_HIP(c, hipEventRecord(f.timers[kTimerLaunch].e0, fs));
        if (rows ? L.dispatch_rows() : L.dispatch_bricks()) return 1;
    }
    if (f.lastMode == DXV_MODE_SURFACE || f.lastMode == DXV_MODE_REFERENCE_SURFACE) {
        // the surface rule's voxels; in mode 3 the shell behind the solid -- behind whatever this launch rewrote, relaunches (sync_frame)
        // included; the surface's 1s lie outside the bricks a kept queue or a kept memset would skip, so the frame keeps nothing for its
        // next launch
        if (enqueue_surface(c, frame, fs)) return 1;
        f.clearSig = 0; f.queueLenSig = 0;
    }
    if (c->opt.events) DXV_HIP(c, hipEventRecord(f.timers[kTimerLaunch].e1, fs));
    DXV_HIP(c, hipEventRecord(f.evEnd, fs));
    f.timed = c->opt.events != 0;
    f.pending = true;
    return 0;
}


// slices this launch writes: local lz in [0, nzLocal) <-> global z0 + (lz / zBlock) * zPeriod + lz % zBlock
int voxelize_common(dxv_ctx* c, uint32_t N, int mode, uint32_t z0, uint32_t nzLocal, uint32_t zBlock, uint32_t zPeriod)
{
    if (!c->haveScene) return fail(c, "dxv_voxelize: no scene (call dxv_build or dxv_scene_import first)");
    if (mode != DXV_MODE_REFERENCE && mode != DXV_MODE_PARITY && mode != DXV_MODE_SURFACE && mode != DXV_MODE_REFERENCE_SURFACE)
        return fail(c, "dxv_voxelize: unknown mode %d", mode);
    if (c->texels && mode != DXV_MODE_REFERENCE) return fail(c, "dxv_voxelize: texel output exists in reference mode only");
    DXV_HIP(c, hipSetDevice(c->device));
    Frame& f = cur_frame(c);
    const hipStream_t fs = cur_stream(c);
    // the frame's previous launch is checked before its grid is reused -- when it can have anything to report: a launch
    // through the lists has no column to run out of, and the next launch simply queues behind it on the frame's stream
    // (no host round trip between back-to-back launches: 20 us of a 0.15 ms launch at 8 ranks)
    if (((f.pending && f.lastCanFail) || f.oct.expandPending) && sync_frame(c, c->cur)) return 1;
    const size_t bytes = (size_t)N * N * nzLocal;
    if (bytes > f.grid.cap) {
        DXV_HIP(c, f.grid.reserve(bytes, align256(bytes), fs));
        f.clearSig = 0;
        f.ptrExposed = false;                                           // (pointers handed out before are dead)
    }
    if (c->texels && bytes > f.texels.cap) {
        DXV_HIP(c, f.texels.reserve(bytes, align256(bytes * 4), fs));
        f.clearSig = 0;
    }
    f.gridBytes = bytes;
    f.grid_dim = N; f.z0 = z0; f.nz = nzLocal;
    f.lastMode = mode; f.lastZBlock = zBlock; f.lastZPeriod = zPeriod;
    grid_rewritten(f);                                                  // (whatever was made of the grid this launch replaces is stale)
    f.drop_unsettled();                                                 // (... and an operator in batches whose verdict nobody has read is dropped with it)
    return launch_now(c, c->cur);
}

// dxv_sync of one frame, the launch's half: wait for its stream, read its status words, redo the launch with a deeper column if asked to
static int sync_launch(dxv_ctx* c, uint32_t i)
{
    Frame& f = c->frames[i];
    const hipStream_t fs = frame_stream(c, i);
    for (int attempt = 0; attempt < 8; ++attempt) {
        // status words and the queue's header in one round trip, into page-locked words
        dxv_ctx::Pinned::PerFrame& pin = c->pin->frame[i];
        uint32_t* words = pin.status;
        const bool readQueue = f.pending && f.lastQueued;
        DXV_HIP(c, hipMemcpyAsync(words, f.status.p, 3 * sizeof(uint32_t), hipMemcpyDeviceToHost, fs));
        if (readQueue) DXV_HIP(c, hipMemcpyAsync(pin.queueLens, f.queue.p + f.queueHdr * kQueueHeaderWords + queue_len_word(0), sizeof(pin.queueLens), hipMemcpyDeviceToHost, fs));
        if (f.oct.expandPending) DXV_HIP(c, hipMemcpyAsync(words + kOctStatusWord, f.status.p + kOctStatusWord, sizeof(uint32_t), hipMemcpyDeviceToHost, fs));
        DXV_HIP(c, hipStreamSynchronize(fs));
        f.sceneReadPending = false;                                     // (whatever read the scene on this stream has finished)
        for (int u = kTimerFirstOperator; u < kTimerFirstBatched; ++u) timer_read(f.timers[u]);     // (the pairs behind them are read where their operators are settled: further batches move their second event)
        read_products(c, i);
        // lists this launch was queued behind without waiting for their verdict: withdrawn -> the launch again, through the tree
        if (settle_lists(c)) return 1;
        if (f.pending && f.usedLists && f.listEpochUsed == c->withdrawnEpoch && c->haveScene && f.grid_dim) {
            f.usedLists = false;
            if (launch_now(c, i, true)) return 1;
            continue;
        }
        const uint32_t status = words[0];
        if (f.pending) {
            f.voxelize_ms = f.timed ? elapsed(f.timers[kTimerLaunch].e0, f.timers[kTimerLaunch].e1) : 0.0f;
            f.redo_rays = f.lastRedoParity < 0 ? 0u : words[1 + f.lastRedoParity];
            if (readQueue) {
                f.plan_bricks = decode_queue_lens(pin.queueLens, f.queueLens);
                f.queueLenSig = f.clearSig;                             // (the queue of this signature: 0 = none kept)
                if (f.lastRebuilt) f.plan_ms = f.timed ? elapsed(f.timers[kTimerQueue].e0, f.timers[kTimerQueue].e1) : 0.0f;
            }
        }
        f.pending = false;
        if (!status) return 0;
        DXV_HIP(c, hipMemsetAsync(f.status.p, 0, sizeof(uint32_t), fs));
        if (!c->opt.stack && c->stackNow < safe_stack(c, ray_rule(f.lastMode)) && c->haveScene && f.grid_dim) {
            // grow to the next instantiated depth (at most up to the depth that cannot overflow) and redo
            const int next = stack_round_up(c->stackNow + 1);
            c->stackNow = next < safe_stack(c, ray_rule(f.lastMode)) ? next : safe_stack(c, ray_rule(f.lastMode));
            if (launch_now(c, i, true)) return 1;
            continue;
        }
        return fail(c, "voxelize kernel reported status 0x%x (traversal stack overflow: tree height %u, stack %u)",
                    status, c->hdr.treeHeight, f.stack_entries);
    }
    return 0;
}

// ... then the halves of the operators that run in batches, and an expansion's verdict (dxv_products.hip)
int sync_frame(dxv_ctx* c, uint32_t i)
{
    if (sync_launch(c, i)) return 1;
    if (settle_fill(c, i)) return 1;
    if (settle_thin(c, i)) return 1;
    if (settle_geodesic(c, i)) return 1;
    if (settle_access(c, i)) return 1;
    return settle_expand(c, i);
}

// The display pass of the selected frame into dst (device memory, rows `pitch` bytes apart), enqueued on the frame's stream behind
// whatever it holds: the empty-brick flags into the frame's own scratch, the ray-cast, the frame's end event behind both (what
// dxv_stream_wait_frame and a refit on another stream wait for).  The caller has checked the frame's grid and the target.
int render_frame(dxv_ctx* c, const RayCastCB& cb, uint32_t width, uint32_t height, uint8_t* dst, size_t pitch, bool timed)
{
    Frame& f = cur_frame(c);
    const hipStream_t fs = cur_stream(c);
    const uint32_t N = f.grid_dim;
    if (c->opt.skipempty) DXV_HIP(c, f.empty.reserve(empty_brick_bytes(N), align256(empty_brick_bytes(N)), fs));     // (only this frame's stream reads the flags)
    DXV_HIP(c, timer_begin(f.timers[kTimerRender], timed, fs));
    DXV_HIP(c, launch_raycast(cb, f.grid.p, N, width, height, dst, pitch, c->opt.skipempty ? f.empty.p : nullptr, fs));
    DXV_HIP(c, timer_end(f.timers[kTimerRender], timed, fs));
    DXV_HIP(c, hipEventRecord(f.evEnd, fs));
    if (c->opt.skipempty) f.emptyDim = N;
    return 0;
}

// dxv_render_async / dxv_stream_wait_frame: the host waits for the selected frame's launch only when that launch can still report
// something -- the rule of dxv_refit: a tree walk whose column can run out (redone with a deeper one), lists that failed their
// deferred check (launched again through the tree).  Anything else is left to the device.
int settle_frame_launch(dxv_ctx* c)
{
    if (settle_lists(c)) return 1;                                     // (waits for a list build's end, not for the launch behind it)
    Frame& f = cur_frame(c);
    if (f.pending && (f.lastCanFail || (f.usedLists && f.listEpochUsed == c->withdrawnEpoch))) return sync_frame(c, c->cur);
    if (f.unsettled()) return sync_frame(c, c->cur);                    // an operator's verdict is not in yet: what is behind it must see the final grid, and further batches go in front of whatever comes now
    return 0;
}

// a whole grid to render: the frame's last launch was neither a slab nor a share
bool frame_renderable(const Frame& f)
{
    const uint32_t N = f.grid_dim;
    return f.grid.p && N && f.z0 == 0 && f.nz == N && f.lastZBlock == N;
}

// memory a caller hands in (dxv_render_async's target, dxv_octree_expand_async's nodes): device memory of this context's device, with the
// whole range inside its allocation
int check_device_range(dxv_ctx* c, const char* who, const void* ptr, size_t need, size_t* room)
{
    hipPointerAttribute_t a{};
    if (hipPointerGetAttributes(&a, ptr) != hipSuccess) {
        (void)hipGetLastError();                                        // (an unknown host pointer is an error of that call: not sticky here)
        return fail(c, "%s: %p is not device memory (host memory is refused)", who, ptr);
    }
    if (a.type != hipMemoryTypeDevice || a.device != c->device)
        return fail(c, "%s: %p is not device memory of device %d (memory type %d, device %d)", who, ptr, c->device, (int)a.type, a.device);
    hipDeviceptr_t base = nullptr;
    size_t size = 0;
    if (hipMemGetAddressRange(&base, &size, const_cast<void*>(ptr)) != hipSuccess) {
        (void)hipGetLastError();
        return fail(c, "%s: no allocation found behind %p", who, ptr);
    }
    const uint8_t* first = static_cast<const uint8_t*>(ptr);
    const size_t offset = (size_t)(first - static_cast<uint8_t*>(base));
    if (first < static_cast<uint8_t*>(base) || offset > size || need > size - offset) {
        *room = offset <= size ? size - offset : (size_t)0;
        return 2;
    }
    return 0;
}

} // namespace dxvhost

extern "C" {

int dxv_update_frame(dxv_ctx* c, const float eye[3], const float viewProj[16], const float posScale[4], uint32_t width, uint32_t height)
{
    if (!c) return 1;
    if (!eye || !viewProj || !width || !height || width > 16384 || height > 16384)
        return fail(c, "dxv_update_frame: bad arguments (eye, view_proj, a viewport of 1 .. 16384 pixels per side)");
    const float unit[4] = {0.0f, 0.0f, 0.0f, 1.0f};                 // DXRVoxelizer.cpp:37
    RayCastCB cb;
    if (!update_frame(c->bound, posScale ? posScale : unit, eye, viewProj, (float)width, (float)height, cb))
        return fail(c, "dxv_update_frame: singular view/projection chain (or no mesh bound yet)");
    Frame& f = cur_frame(c);
    f.cb = cb;
    f.cbWidth = width; f.cbHeight = height;
    return 0;
}

int dxv_render_async(dxv_ctx* c, void* deviceRgba, size_t rowPitch)
{
    if (!c) return 1;
    Frame& f = cur_frame(c);
    if (!f.cbWidth) return fail(c, "dxv_render_async: frame %u has no ray-cast constants (call dxv_update_frame first)", c->cur);
    if (!frame_renderable(f))
        return fail(c, "dxv_render_async: needs the whole grid of the frame's last launch (z0 = 0, nz = grid_dim), not a slab or a share");
    const uint32_t w = f.cbWidth, h = f.cbHeight;
    if (!deviceRgba || rowPitch < (size_t)w * 4 || rowPitch % 4 || reinterpret_cast<uintptr_t>(deviceRgba) % 4)
        return fail(c, "dxv_render_async: target %p with row pitch %zu: need a 4-byte aligned pointer and a pitch that is a multiple of 4 "
                       "and at least width * 4 = %zu", deviceRgba, rowPitch, (size_t)w * 4);
    DXV_HIP(c, hipSetDevice(c->device));
    const size_t need = (size_t)(h - 1) * rowPitch + (size_t)w * 4;
    size_t room = 0;
    if (const int r = check_device_range(c, "dxv_render_async", deviceRgba, need, &room))
        return r == 1 ? 1 : fail(c, "dxv_render_async: %u x %u texels at pitch %zu need %zu bytes, the allocation behind %p has %zu", w, h, rowPitch, need, deviceRgba, room);
    if (settle_frame_launch(c)) return 1;
    return render_frame(c, f.cb, w, h, static_cast<uint8_t*>(deviceRgba), rowPitch, c->opt.events != 0);
}

int dxv_stream_wait_frame(dxv_ctx* c, void* hipStream)
{
    if (!c) return 1;
    DXV_HIP(c, hipSetDevice(c->device));
    if (settle_frame_launch(c)) return 1;
    DXV_HIP(c, hipStreamWaitEvent(static_cast<hipStream_t>(hipStream), cur_frame(c).evEnd, 0));
    return 0;
}

int dxv_voxelize_async(dxv_ctx* c, uint32_t N, int mode, uint32_t z0, uint32_t nz)
{
    if (!c) return 1;
    if (check_slab(c, "dxv_voxelize", N, z0, nz)) return 1;
    return voxelize_common(c, N, mode, z0, nz, nz, nz);
}

int dxv_voxelize_interleaved_async(dxv_ctx* c, uint32_t N, int mode, uint32_t rank, uint32_t world, uint32_t zblock)
{
    if (!c) return 1;
    if (check_grid(c, "dxv_voxelize", N) || check_interleave(c, "dxv_voxelize_interleaved", N, rank, world, zblock)) return 1;
    return voxelize_common(c, N, mode, rank * zblock, N / world, zblock, zblock * world);
}

int dxv_prepare_launch(dxv_ctx* c, uint32_t N, uint32_t z0, uint32_t nz)
{
    if (!c) return 1;
    if (check_slab(c, "dxv_prepare_launch", N, z0, nz)) return 1;
    return prepare_partition(c, N, z0, nz, nz, nz);
}

int dxv_prepare_launch_interleaved(dxv_ctx* c, uint32_t N, uint32_t rank, uint32_t world, uint32_t zblock)
{
    if (!c) return 1;
    if (check_grid(c, "dxv_prepare_launch", N) || check_interleave(c, "dxv_prepare_launch_interleaved", N, rank, world, zblock)) return 1;
    return prepare_partition(c, N, rank * zblock, N / world, zblock, zblock * world);
}

int dxv_voxelize_interleaved(dxv_ctx* c, uint32_t N, int mode, uint32_t rank, uint32_t world, uint32_t zblock)
{
    if (dxv_voxelize_interleaved_async(c, N, mode, rank, world, zblock)) return 1;
    return dxv_sync(c);
}

int dxv_sync(dxv_ctx* c)
{
    if (!c) return 1;
    DXV_HIP(c, hipSetDevice(c->device));
    return sync_frame(c, c->cur);
}

int dxv_sync_all(dxv_ctx* c)
{
    if (!c) return 1;
    DXV_HIP(c, hipSetDevice(c->device));
    return sync_frames(c);
}

int dxv_voxelize(dxv_ctx* c, uint32_t N, int mode, uint32_t z0, uint32_t nz)
{
    if (dxv_voxelize_async(c, N, mode, z0, nz)) return 1;
    return dxv_sync(c);
}

} // extern "C"
