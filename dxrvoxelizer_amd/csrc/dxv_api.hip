// dxv_api.hip -- the C-ABI of libdxv.so (include/dxv.h): context, device memory, mesh, build and refit, results,
// options.  The other entry points: dxv_frames.hip (launches), dxv_products.hip (what is made of a frame's grid), dxv_lists.hip
// (candidate lists), dxv_blob.hip (scene blob), dxv_debug.hip (test hooks).  There is no CPU fallback anywhere in this library: without a HIP device dxv_create fails.
#include "dxv_ctx.h"
#include <chrono>

using namespace dxv;
using namespace dxvhost;

namespace {
thread_local std::string g_createError;
}

namespace dxvhost {

int fail(dxv_ctx* c, const char* fmt, ...)
{
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    if (c) c->err = buf; else g_createError = buf;
    return 1;
}

void layout_scene(SceneHeader& h, uint32_t T, uint32_t V, bool wide)
{
    memset(&h, 0, sizeof(h));
    h.magic = kSceneMagic;
    h.version = kSceneVersion;
    h.numTris = T;
    h.numVerts = V;
    h.numNodes = T > 1 ? T - 1 : 1;
    h.offNodes = align256(sizeof(SceneHeader));
    h.offNodes32 = align256(h.offNodes + sizeof(Node) * (size_t)h.numNodes);
    h.offNodes64 = align256(h.offNodes32 + sizeof(Node32) * (size_t)h.numNodes);
    h.hasWide = wide ? 1u : 0u;
    h.offTriPos = align256(h.offNodes64 + (wide ? sizeof(Node64) * (size_t)h.numNodes : 0));
    h.offTriNrm = align256(h.offTriPos + sizeof(TriPos) * (size_t)T);
    h.totalBytes = align256(h.offTriNrm + sizeof(TriNrm) * (size_t)T);
}

int alloc_scene(dxv_ctx* c, uint32_t T, uint32_t V, bool wide)
{
    SceneHeader h;
    layout_scene(h, T, V, wide);
    DXV_HIP(c, c->scene.fit(h.totalBytes));
    c->sceneBytes = h.totalBytes;
    c->hdr = h;
    return 0;
}

int alloc_scratch(dxv_ctx* c, uint32_t T)
{
    BuildScratch& s = c->scratch;
    if (s.T == T) return 0;
    // (scratch made for a mesh of up to twice the triangles serves this one too)
    if (s.keys.cap >= T && s.keys.cap / 2 <= T && radix_sort_hist_words(T) <= s.hist.cap) {
        if (s.pyramid.cap < pyramid_slots(T)) s.pyramid.release();     // (alloc_pyramid makes the larger one)
        s.T = T;
        return 0;
    }
    s = BuildScratch{};
    const size_t n = T, hist = radix_sort_hist_words(T);
    hipError_t e = s.keys.reserve(n, sizeof(uint64_t) * n);
    if (e == hipSuccess) e = s.keysTmp.reserve(n, sizeof(uint64_t) * n);
    if (e == hipSuccess) e = s.hist.reserve(hist, sizeof(uint32_t) * hist);
    if (e == hipSuccess) e = s.parents.reserve(2 * n, sizeof(uint32_t) * 2 * n);
    if (e == hipSuccess) e = s.flags.reserve(n, sizeof(uint32_t) * n);
    if (e == hipSuccess) e = s.flags2.reserve(n, sizeof(uint32_t) * n);
    if (e != hipSuccess) {
        s = BuildScratch{};                                             // (all of it or none: what is kept is judged by the keys' capacity)
        return fail(c, "build scratch: hipMalloc failed: %s", hipGetErrorString(e));
    }
    s.T = T;
    return 0;
}

// What a new mesh, a build, a refit or an import invalidates: the scene, everything derived from it (lists, row lists, prepared
// queues, the launch history the lists' policy reads) -- and, depending on the cause, mesh and hierarchy.
void scene_changed(dxv_ctx* c, SceneCause why)
{
    drop_prepared(c);
    c->haveScene = false;
    c->lists.state = 0; c->specRes = 0; c->listResFloor = 0; c->listFloorTried = false; c->launchesOfScene = 0;
    c->rowLists.state = 0; c->parityLaunchesOfScene = 0;
    // a refit keeps the hierarchy it works on (what it leaves stale it says itself) and marks the mesh as animated
    c->refitted = why == SceneCause::refit;
    if (why != SceneCause::refit) { c->haveHierarchy = false; c->nodesStale = 0; }
    // a new mesh and an imported scene replace the resident mesh (dxv_set_mesh has it back when its upload succeeds)
    if (why == SceneCause::mesh || why == SceneCause::import) c->haveMesh = false;
    if (why == SceneCause::mesh) c->vbCopyQueued = false;           // (build and refit: finish_build, once the copy has been waited for)
}

void fill_scene_stats(dxv_ctx* c)
{
    c->stats.num_tris = c->hdr.numTris; c->stats.num_verts = c->hdr.numVerts; c->stats.num_nodes = c->hdr.numNodes;
    c->stats.tree_height = c->hdr.treeHeight;
    c->stats.tri_extent = c->hdr.triExtent;
    memcpy(c->stats.bound, c->bound, sizeof(c->bound));
}

// dxv_set_mesh's look at the caller's arrays: largest index, position bounds, whether every position is finite.  Chunks of the
// arrays go to up to eight threads; the chunks' results are merged in order with the strict comparisons of a sequential sweep, so
// the bounds are the sequential sweep's bit for bit (signs of zero included).
struct MeshScan { uint32_t maxIndex; float mn[3], mx[3]; bool finite; };
static void scan_mesh_range(const float* vb, size_t v0, size_t v1, const uint32_t* ib, size_t i0, size_t i1, MeshScan* out)
{
    uint32_t m = 0;
    for (size_t i = i0; i < i1; ++i) m = ib[i] > m ? ib[i] : m;
    float mn[3] = {INFINITY, INFINITY, INFINITY}, mx[3] = {-INFINITY, -INFINITY, -INFINITY}, probe = 0.0f;
    for (size_t v = v0; v < v1; ++v) {
        const float* p = vb + 6 * v;
        for (int a = 0; a < 3; ++a) {
            mn[a] = p[a] < mn[a] ? p[a] : mn[a];
            mx[a] = p[a] > mx[a] ? p[a] : mx[a];
            probe += p[a] - p[a];                 // 0 for every finite value, NaN for NaN and +-Inf
        }
    }
    out->maxIndex = m;
    for (int a = 0; a < 3; ++a) { out->mn[a] = mn[a]; out->mx[a] = mx[a]; }
    out->finite = probe == 0.0f;
}
static MeshScan scan_mesh(const float* vb, uint32_t V, const uint32_t* ib, uint32_t T)
{
    const size_t nIdx = 3 * (size_t)T;
    unsigned hw = std::thread::hardware_concurrency();
    // (a thread per quarter of a million elements, up to eight: starting and joining one costs ~50 us, as much as it sweeps in that time --
    // the bunny's 245 k elements went from 0.2 to 0.36 ms with eight)
    unsigned nt = (unsigned)((nIdx + V) / 250000u);
    nt = nt < 1u ? 1u : nt > 8u ? 8u : nt;
    if (hw && nt > hw) nt = hw;
    if (nt > V) nt = 1;
    MeshScan part[8];
    std::thread th[8];
    unsigned started = 1;
    auto lo = [&](size_t n, unsigned k) { return n * k / nt; };
    for (unsigned k = 1; k < nt; ++k) {
        try { th[k] = std::thread(scan_mesh_range, vb, lo(V, k), lo(V, k + 1), ib, lo(nIdx, k), lo(nIdx, k + 1), &part[k]); ++started; }
        catch (...) { break; }                 // (no thread to be had: the caller's thread does the rest)
    }
    if (started < nt) {                        // what the threads that did not start would have covered
        scan_mesh_range(vb, lo(V, started), V, ib, lo(nIdx, started), nIdx, &part[started]);
        for (unsigned k = started + 1; k < nt; ++k) { part[k] = part[started]; }
    }
    scan_mesh_range(vb, 0, lo(V, 1), ib, 0, lo(nIdx, 1), &part[0]);
    for (unsigned k = 1; k < started; ++k) th[k].join();
    MeshScan r = part[0];
    for (unsigned k = 1; k < nt; ++k) {
        r.maxIndex = part[k].maxIndex > r.maxIndex ? part[k].maxIndex : r.maxIndex;
        for (int a = 0; a < 3; ++a) {
            if (part[k].mn[a] < r.mn[a]) r.mn[a] = part[k].mn[a];
            if (part[k].mx[a] > r.mx[a]) r.mx[a] = part[k].mx[a];
        }
        r.finite = r.finite && part[k].finite;
    }
    return r;
}

} // namespace dxvhost

extern "C" {

int dxv_create(dxv_ctx** out, int device)
{
    if (!out) return fail(nullptr, "dxv_create: out is NULL");
    *out = nullptr;
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess || n <= 0)
        return fail(nullptr, "dxv_create: no HIP device available (%s); this library has no CPU path",
                    e != hipSuccess ? hipGetErrorString(e) : "device count 0");
    if (device < 0 || device >= n) return fail(nullptr, "dxv_create: device %d out of range [0,%d)", device, n);
    dxv_ctx* c = new dxv_ctx();
    c->device = device;
    if (hipSetDevice(device) != hipSuccess || hipStreamCreateWithFlags(&c->ownStream, hipStreamNonBlocking) != hipSuccess) {
        delete c;
        return fail(nullptr, "dxv_create: cannot initialise device %d", device);
    }
    c->stream = c->ownStream;
    for (auto& ev : c->ev) {
        if (hipEventCreate(&ev) != hipSuccess) { delete c; return fail(nullptr, "dxv_create: hipEventCreate failed"); }
    }
    for (auto& ev : c->evList) {
        if (hipEventCreate(&ev) != hipSuccess) { dxv_destroy(c); return fail(nullptr, "dxv_create: hipEventCreate failed"); }
    }
    if (hipHostMalloc(reinterpret_cast<void**>(&c->pin), sizeof(dxv_ctx::Pinned), hipHostMallocDefault) != hipSuccess) {
        c->pin = nullptr;
        dxv_destroy(c);
        return fail(nullptr, "dxv_create: hipHostMalloc failed");
    }
    memset(c->pin, 0, sizeof(dxv_ctx::Pinned));
    if (c->count.reserve(32, 256) != hipSuccess || c->rootInfo.reserve(64, 256) != hipSuccess || frame_prepare(c, 0)) {
        dxv_destroy(c);
        return fail(nullptr, "dxv_create: hipMalloc failed");
    }
    *out = c;
    // A process's first build and first launch on a device pay for what the runtime sets up lazily (dxv_warmup, below): the first
    // context of a process on a device runs that pass once (DXV_WARMUP=0: not at all) and says in its stats what it cost.
    const char* wu = getenv("DXV_WARMUP");
    if (!(wu && wu[0] == '0')) (void)dxv_warmup(device, &c->stats.warmup_ms);
    return 0;
}

// The code object of the library, the first host-to-device copy's staging, every kernel's first dispatch: 11 ms for the first Init of a
// 1 M-triangle mesh against 3.3 for one that follows anything at all (LBVH 1.3 against 0.29 ms, lists 1.6 against 0.95, upload 7
// against 0.7).  This sends a four-triangle scene through every step once, on a context of its own that is gone when it returns.
// Once per process and device; errors of the pass are nobody's (the caller's own calls will report theirs), and the error state the
// caller sees is left as it was.
int dxv_warmup(int device, float* ms)
{
    static std::atomic<uint64_t> warmed{0};
    if (ms) *ms = 0.0f;
    if (device < 0) return 1;
    const uint64_t bit = 1ull << (device & 63);
    if (warmed.fetch_or(bit) & bit) return 0;
    const std::string keep = g_createError;
    const auto t0 = std::chrono::steady_clock::now();
    dxv_ctx* w = nullptr;
    if (dxv_create(&w, device) == 0) {                                 // (its own call of this function finds the device marked)
        static const float vb[4 * 6] = {0.9f, 0.9f, 0.9f, 0.58f, 0.58f, 0.58f,   -0.9f, -0.9f, 0.9f, -0.58f, -0.58f, 0.58f,
                                        -0.9f, 0.9f, -0.9f, -0.58f, 0.58f, -0.58f,   0.9f, -0.9f, -0.9f, 0.58f, -0.58f, -0.58f};
        static const uint32_t ib[4 * 3] = {0, 1, 2, 0, 3, 1, 0, 2, 3, 1, 3, 2};
        if (dxv_set_mesh(w, vb, 4, ib, 4) == 0 && dxv_build(w) == 0 && dxv_build_lists_for_grid(w, 32) == 0) {
            (void)dxv_voxelize(w, 32, DXV_MODE_REFERENCE, 0, 32);       // (through the prepared queue)
            (void)dxv_set_option(w, "prepared", 0);
            (void)dxv_voxelize(w, 32, DXV_MODE_REFERENCE, 0, 32);       // (through a queue of its own)
            (void)dxv_voxelize(w, 32, DXV_MODE_PARITY, 0, 32);
            (void)dxv_voxelize(w, 32, DXV_MODE_SURFACE, 0, 32);
            std::vector<uint8_t> host(32 * 32 * 32);
            (void)dxv_grid_download(w, host.data(), host.size());
        }
        std::vector<uint8_t> mb(1u << 20);                       // (a copy of a size the staging path handles in pieces)
        DevBuf<uint8_t> d;
        if (d.reserve(mb.size(), mb.size()) == hipSuccess) (void)hipMemcpy(d.p, mb.data(), mb.size(), hipMemcpyHostToDevice);
        dxv_destroy(w);
    }
    (void)hipGetLastError();
    g_createError = keep;
    if (ms) *ms = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t0).count();
    return 0;
}

void dxv_destroy(dxv_ctx* c)
{
    if (!c) return;
    (void)hipSetDevice(c->device);
    for (uint32_t i = 0; i < DXV_FRAME_COUNT; ++i) {
        Frame& f = c->frames[i];
        if (frame_stream(c, i)) (void)hipStreamSynchronize(frame_stream(c, i));
        for (Timer& t : f.timers)
            for (hipEvent_t ev : {t.e0, t.e1})
                if (ev) (void)hipEventDestroy(ev);
        if (f.evEnd) (void)hipEventDestroy(f.evEnd);
        if (f.ownStream) (void)hipStreamDestroy(f.ownStream);
    }
    for (auto& ev : c->ev) if (ev) (void)hipEventDestroy(ev);
    for (auto& ev : c->evList) if (ev) (void)hipEventDestroy(ev);
    if (c->pin) (void)hipHostFree(c->pin);
    if (c->copyStream) (void)hipStreamDestroy(c->copyStream);
    if (c->ownStream) (void)hipStreamDestroy(c->ownStream);
    delete c;                                                           // (every device buffer is a member that frees itself: DevBuf)
}

int dxv_api_version(void) { return DXV_API_VERSION; }

int dxv_trim(dxv_ctx* c)
{
    if (!c) return 1;
    DXV_HIP(c, hipSetDevice(c->device));
    if (sync_frames(c)) return 1;
    DXV_HIP(c, hipStreamSynchronize(c->stream));
    c->listScratchA.release(); c->listScratchB.release();
    for (auto& f : c->frames) f.trim_products();                        // (the scratch of every operator; what they made of the grid stays: Frame)
    c->specRes = 0;
    if (!c->haveHierarchy) c->scratch = BuildScratch{};                             // (a built scene keeps keys and links: dxv_refit reads them)
    // prepared queues of lists that are gone (their slots keep their memory for the next dxv_prepare_launch of the partition: 8 MB at
    // 512^3, half a gigabyte at 2048^3); the ones in use stay
    for (auto& q : c->prepared)
        if (q.epoch != c->listEpoch || c->lists.state != 1) q = dxv_ctx::Prepared{};
    return 0;
}

const char* dxv_last_error(const dxv_ctx* c) { return c ? c->err.c_str() : g_createError.c_str(); }

int dxv_set_stream(dxv_ctx* c, void* s)
{
    if (!c) return 1;
    DXV_HIP(c, hipSetDevice(c->device));
    if (sync_frames(c)) return 1;
    DXV_HIP(c, hipStreamSynchronize(c->stream));
    c->stream = s ? static_cast<hipStream_t>(s) : c->ownStream;
    return 0;
}

int dxv_set_frame(dxv_ctx* c, uint32_t frame)
{
    if (!c) return 1;
    if (frame >= DXV_FRAME_COUNT) return fail(c, "dxv_set_frame: frame %u out of range [0, %d)", frame, DXV_FRAME_COUNT);
    DXV_HIP(c, hipSetDevice(c->device));
    if (frame_prepare(c, frame)) return 1;
    c->cur = frame;
    return 0;
}

int dxv_set_mesh(dxv_ctx* c, const float* vb, uint32_t V, const uint32_t* ib, uint32_t T)
{
    if (!c) return 1;
    if (!vb || !ib || !V || !T) return fail(c, "dxv_set_mesh: empty mesh (V=%u, T=%u)", V, T);
    if (T > 0x7fffffffu / 2) return fail(c, "dxv_set_mesh: too many triangles (%u)", T);
    // One sweep over the caller's arrays, in up to eight threads: the largest index, and the AABB over every VB position
    // (XUSGObjLoader.cpp:386-416) -- branch-free, so the compiler vectorises the index half; the slow loops that name the
    // offending element run only when the sweep has found one.  Centre and half max extent: Content/Voxelizer.cpp:52-57.
    const MeshScan scan = scan_mesh(vb, V, ib, T);
    if (scan.maxIndex >= V)
        for (size_t i = 0; i < 3 * (size_t)T; ++i)
            if (ib[i] >= V) return fail(c, "dxv_set_mesh: index %u at position %zu out of range (V=%u)", ib[i], i, V);
    if (!scan.finite)
        for (uint32_t i = 0; i < V; ++i) {
            const float* p = vb + 6 * (size_t)i;
            if (!std::isfinite(p[0]) || !std::isfinite(p[1]) || !std::isfinite(p[2]))
                return fail(c, "dxv_set_mesh: vertex %u has a non-finite position (%g, %g, %g)", i, (double)p[0], (double)p[1], (double)p[2]);
        }
    const float* mn = scan.mn;
    const float* mx = scan.mx;
    const float ex = mx[0] - mn[0], ey = mx[1] - mn[1], ez = mx[2] - mn[2];
    // (into locals: a mesh that is refused leaves the context's earlier mesh AND its bound alone -- a later dxv_refit / dxv_build of
    // that mesh normalises with the bound it was set with)
    const float eyz = ey > ez ? ey : ez;
    const float bound[4] = {(mx[0] + mn[0]) / 2.0f, (mx[1] + mn[1]) / 2.0f, (mx[2] + mn[2]) / 2.0f, (ex > eyz ? ex : eyz) / 2.0f};
    if (!(bound[3] > 0.0f) || !std::isfinite(bound[3]) || !std::isfinite(bound[0]) || !std::isfinite(bound[1]) || !std::isfinite(bound[2]))
        return fail(c, "dxv_set_mesh: degenerate or non-finite bound (half extent %g)", (double)bound[3]);

    DXV_HIP(c, hipSetDevice(c->device));
    if (sync_frames(c)) return 1;
    DXV_HIP(c, hipStreamSynchronize(c->stream));
    memcpy(c->bound, bound, sizeof(bound));
    scene_changed(c, SceneCause::mesh);
    // (a mesh of the size of the last one moves into its buffers: two frees and two allocations less on the way to the first launch)
    const size_t vbBytes = sizeof(float) * 6 * (size_t)V, ibBytes = sizeof(uint32_t) * 3 * (size_t)T;
    DXV_HIP(c, c->vb.fit(vbBytes));
    DXV_HIP(c, c->ib.fit(ibBytes));
    DXV_HIP(c, hipEventRecord(c->ev[8], c->stream));
    DXV_HIP(c, hipMemcpyAsync(c->vb.p, vb, vbBytes, hipMemcpyHostToDevice, c->stream));
    DXV_HIP(c, hipMemcpyAsync(c->ib.p, ib, ibBytes, hipMemcpyHostToDevice, c->stream));
    DXV_HIP(c, hipEventRecord(c->ev[9], c->stream));
    DXV_HIP(c, hipStreamSynchronize(c->stream));
    c->T = T; c->V = V;
    c->haveMesh = true;
    c->stats.num_tris = T; c->stats.num_verts = V;
    memcpy(c->stats.bound, c->bound, sizeof(c->bound));
    c->stats.upload_ms = elapsed(c->ev[8], c->ev[9]);
    return 0;
}

} // extern "C"

namespace dxvhost {
void fill_build_buffers(dxv_ctx* c, BuildBuffers& b)
{
    const BuildScratch& s = c->scratch;
    b.vb = c->vb.p; b.ib = c->ib.p; b.T = c->T; b.V = c->V;
    memcpy(b.bound, c->bound, sizeof(c->bound));
    b.keys = s.keys.p; b.keysTmp = s.keysTmp.p; b.hist = s.hist.p; b.parents = s.parents.p;
    b.flags = s.flags.p; b.flags2 = s.flags2.p; b.rootInfo = c->rootInfo.p; b.pyramid = s.pyramid.p;
    b.nodes = scene_nodes(c); b.nodes32 = scene_nodes32(c); b.nodes64 = c->hdr.hasWide ? scene_nodes64(c) : nullptr; b.triPos = scene_tripos(c); b.triNrm = scene_trinrm(c);
}

// The half-float / four-box copies of the hierarchy after a refit that skipped them (dxv_refit): made now, on `stream`, and
// finished before anyone else can launch a walk on another stream.
int wait_scene_readers(dxv_ctx* c, hipStream_t stream)
{
    for (uint32_t i = 0; i < DXV_FRAME_COUNT; ++i) {
        Frame& f = c->frames[i];
        if (f.ready && f.sceneReadPending && frame_stream(c, i) != stream) DXV_HIP(c, hipStreamWaitEvent(stream, f.evEnd, 0));
    }
    return 0;
}

int ensure_nodes(dxv_ctx* c, hipStream_t stream)
{
    if (!c->nodesStale) return 0;
    if (wait_scene_readers(c, stream)) return 1;                        // (a mesh distance walk of another frame may still read the boxes)
    BuildBuffers b{};
    fill_build_buffers(c, b);
    if (c->nodesStale == 2) DXV_HIP(c, lbvh_refit_boxes(b, stream));
    else DXV_HIP(c, lbvh_traversal_copies(b, stream));
    DXV_HIP(c, hipStreamSynchronize(stream));
    c->nodesStale = 0;
    return 0;
}

// min/max pyramid of the box merge (refit = 1): 24 B box + 4 B deepest leaf per slot
int alloc_pyramid(dxv_ctx* c)
{
    if (!c->scratch.pyramid.p && c->opt.refit == 1 && c->T > 1)     // refit=2 keeps the level sweeps, refit=0 the atomic pass
        DXV_HIP(c, c->scratch.pyramid.reserve(pyramid_slots(c->T), 28 * (size_t)pyramid_slots(c->T)));
    return 0;
}

// headerToDevice: the resident copy of the header (nothing on the device reads it -- launches get their words through kernel
// arguments, an export writes the blob's header from the host's copy): dxv_build keeps it current, a refit saves the round trip
int finish_build(dxv_ctx* c, const char* who, bool headerToDevice = true)
{
    uint32_t* rootInfo = c->pin->rootInfo;
    DXV_HIP(c, hipMemcpyAsync(rootInfo, c->rootInfo.p, sizeof(c->pin->rootInfo), hipMemcpyDeviceToHost, c->stream));
    DXV_HIP(c, hipStreamSynchronize(c->stream));
    c->vbCopyQueued = false;
    if (rootInfo[7] != 1) return fail(c, "%s: did not complete", who);
    if (rootInfo[11]) return fail(c, "%s: %u triangle(s) have a non-finite vertex position (NaN / Inf in the vertex buffer)", who, rootInfo[11]);
    memcpy(c->hdr.rootLo, &rootInfo[0], 12);
    memcpy(c->hdr.rootHi, &rootInfo[3], 12);
    c->hdr.treeHeight = rootInfo[6];
    if (rootInfo[10]) {   // k_tri_keys: sum over the sampled triangles of (extent y + extent z) in 2^-20 units, and their number
        unsigned long long ext;
        memcpy(&ext, &rootInfo[8], sizeof(ext));
        c->hdr.triExtent = (float)((double)ext / 1048576.0 / 2.0 / (double)rootInfo[10]);
    }                     // (a refit keeps the figure of the build)
    for (int a = 0; a < 3; ++a)
        if (!(c->hdr.rootLo[a] <= c->hdr.rootHi[a]))
            return fail(c, "%s: refit produced an invalid root box (axis %d: %g > %g)", who, a,
                        (double)c->hdr.rootLo[a], (double)c->hdr.rootHi[a]);
    if (c->hdr.treeHeight == 0 || c->hdr.treeHeight > 64) return fail(c, "%s: implausible tree height %u", who, c->hdr.treeHeight);
    if (headerToDevice) {
        DXV_HIP(c, hipMemcpyAsync(c->scene.p, &c->hdr, sizeof(SceneHeader), hipMemcpyHostToDevice, c->stream));
        DXV_HIP(c, hipStreamSynchronize(c->stream));
    }
    c->haveScene = true;
    ++c->sceneEpoch;
    c->stackNow = initial_stack(c);
    fill_scene_stats(c);
    return 0;
}
} // namespace dxvhost

extern "C" {

int dxv_update_vertices(dxv_ctx* c, const float* vb, uint32_t V)
{
    if (!c) return 1;
    if (!c->haveMesh || !c->vb.p) return fail(c, "dxv_update_vertices: no mesh resident on this context");
    if (!vb || V != c->V) return fail(c, "dxv_update_vertices: vertex count must stay %u, got %u", c->V, V);
    DXV_HIP(c, hipSetDevice(c->device));
    // No wait for the frames: their launches read the scene's triangle records and lists, never the vertex buffer -- its only
    // readers are dxv_build and dxv_refit, which return after their work is done.  The upload therefore runs on a stream of its
    // own, beside whatever the frames still have in flight (12 MB over PCIe at 1 M triangles: 0.25 ms hidden behind a launch).
    if (!c->copyStream) DXV_HIP(c, hipStreamCreateWithFlags(&c->copyStream, hipStreamNonBlocking));
    if (c->vbCopyQueued) { DXV_HIP(c, hipStreamSynchronize(c->stream)); c->vbCopyQueued = false; }    // (an earlier device update lands first)
    DXV_HIP(c, hipMemcpyAsync(c->vb.p, vb, sizeof(float) * 6 * (size_t)V, hipMemcpyHostToDevice, c->copyStream));
    DXV_HIP(c, hipStreamSynchronize(c->copyStream));
    return 0;
}

int dxv_update_vertices_device(dxv_ctx* c, const void* dvb, uint32_t V)
{
    if (!c) return 1;
    if (!c->haveMesh || !c->vb.p) return fail(c, "dxv_update_vertices_device: no mesh resident on this context");
    if (!dvb || V != c->V) return fail(c, "dxv_update_vertices_device: vertex count must stay %u, got %u", c->V, V);
    DXV_HIP(c, hipSetDevice(c->device));
    // No wait for the frames (as in dxv_update_vertices): their launches never read the vertex buffer, and its readers --
    // dxv_build, dxv_refit -- run on this same stream.
    DXV_HIP(c, hipMemcpyAsync(c->vb.p, dvb, sizeof(float) * 6 * (size_t)V, hipMemcpyDeviceToDevice, c->stream));
    c->vbCopyQueued = true;
    return 0;                                                          // (dxv_refit, on the same stream, comes next)
}

int dxv_refit(dxv_ctx* c)
{
    if (!c) return 1;
    if (!c->haveMesh || !c->haveHierarchy || c->scratch.T != c->T || !c->T)
        return fail(c, "dxv_refit: needs a scene built on this context by dxv_build (imported scenes carry no build state)");
    DXV_HIP(c, hipSetDevice(c->device));
    // The frames' launches read what the refit is about to write.  A launch that may still have something to say (a tree walk whose
    // column can run out; lists that failed their deferred check) is synchronised on the host and, if need be, run again against
    // the OLD scene; every other launch is waited for ON THE DEVICE -- frame 0 shares this stream, the other frames' end events
    // are waited for by it -- so that the refit's kernels, the lists' counting pass and the host's one synchronisation of the
    // frame (finish_build) queue up behind a launch that is still running.
    if (settle_lists(c)) return 1;                                     // (waits for a build's end, not for the launch behind it)
    for (uint32_t i = 0; i < DXV_FRAME_COUNT; ++i) {
        Frame& f = c->frames[i];
        if (!f.ready || !f.pending) continue;
        if (f.lastCanFail || (f.usedLists && f.listEpochUsed == c->withdrawnEpoch)) { if (sync_frame(c, i)) return 1; }
        else if (frame_stream(c, i) != c->stream) DXV_HIP(c, hipStreamWaitEvent(c->stream, f.evEnd, 0));
    }
    // ... and so is a pass behind a launch that reads nodes and triangle records (dxv_mesh_distance_async), whether or not the
    // launch itself has been checked since: the frame's end event lies behind it
    if (wait_scene_readers(c, c->stream)) return 1;
    const uint32_t hadListsOn = c->lists.state == 1 ? c->lists.res : 0u;
    scene_changed(c, SceneCause::refit);                               // (the queues prepared for the old surface go too; no launch that reads one is un-ordered: see above)
    if (alloc_pyramid(c)) return 1;
    BuildBuffers b{};
    fill_build_buffers(c, b);
    if (c->opt.refit != 1) b.pyramid = nullptr;
    // the wide walks' four-box copy of the hierarchy waits until a walk needs it: the next launch of a refitted mesh usually
    // goes through the lists, which are built from the triangle records alone (the half-float copy comes out of the box
    // merge's registers and is always current)
    b.deferCopies = c->opt.lists != 0 && c->hdr.hasWide;
    // ... and so do the node boxes themselves (half of the refit's time at 1 M triangles): the refit stops at the min/max
    // pyramid, whose top is the root box the launch needs, and ensure_nodes finishes it in front of the first tree walk
    b.deferBoxes = c->opt.lists != 0 && c->opt.deferboxes && b.pyramid && c->T > 1;
    DXV_HIP(c, lbvh_refit(b, c->opt.refit, c->hdr.treeHeight, c->stream, c->ev + 3));
    c->nodesStale = b.deferBoxes ? 2 : b.deferCopies ? 1 : 0;
    // A scene that had lists (or asks for them from its first launch) will have them rebuilt by its next launch: their counting
    // pass needs the new triangle records only, so it runs here, behind the refit, and its total comes back with the root box.
    uint32_t spec = 0;
    if (c->opt.lists && (hadListsOn || c->opt.lists == 2) && c->listScratchA.cap >= list_scratch_a(nullptr, c->hdr.numTris).bytes) {
        spec = c->opt.listres ? (uint32_t)c->opt.listres : list_resolution(c);     // (the base map: a mesh that is being refitted gets its lists built for one launch)
        const ListScratchA sa = list_scratch_a(c->listScratchA.p, c->hdr.numTris);
        DXV_HIP(c, hipEventRecord(c->evList[0], c->stream));
        DXV_HIP(c, dirmap_count(scene_tripos(c), c->hdr.numTris, spec, sa.rec, sa.counts, sa.pairs, sa.offsets, sa.total, c->opt.lateralpad != 0, c->stream));
        DXV_HIP(c, hipEventRecord(c->evList[1], c->stream));
        DXV_HIP(c, hipMemcpyAsync(&c->pin->listTotal, sa.total, sizeof(unsigned long long), hipMemcpyDeviceToHost, c->stream));
    }
    if (finish_build(c, "dxv_refit", false)) return 1;
    c->specRes = spec;
    c->stats.refit_ms = elapsed(c->ev[3], c->ev[4]);
    return 0;
}

int dxv_build(dxv_ctx* c)
{
    if (!c) return 1;
    if (!c->haveMesh) return fail(c, "dxv_build: no mesh (call dxv_set_mesh first)");
    DXV_HIP(c, hipSetDevice(c->device));
    if (sync_frames(c)) return 1;
    scene_changed(c, SceneCause::build);
    if (alloc_scene(c, c->T, c->V, c->opt.wide != 0)) return 1;
    if (alloc_scratch(c, c->T)) return 1;
    if (alloc_pyramid(c)) return 1;
    memcpy(c->hdr.bound, c->bound, sizeof(c->bound));

    BuildBuffers b{};
    fill_build_buffers(c, b);
    if (c->opt.refit != 1) b.pyramid = nullptr;
    b.deferCopies = c->opt.lists != 0 && c->hdr.hasWide;                // (as in dxv_refit: 0.6 ms of a 10 M-triangle build that most scenes never need)
    DXV_HIP(c, lbvh_build(b, c->opt.refit, c->stream, c->ev));
    c->nodesStale = b.deferCopies ? 1 : 0;
    if (finish_build(c, "dxv_build")) return 1;
    c->haveHierarchy = true;
    c->stats.prep_ms = elapsed(c->ev[0], c->ev[1]);
    c->stats.sort_ms = elapsed(c->ev[1], c->ev[2]);
    c->stats.hierarchy_ms = elapsed(c->ev[2], c->ev[3]);
    c->stats.refit_ms = elapsed(c->ev[3], c->ev[4]);
    c->stats.build_ms = elapsed(c->ev[0], c->ev[4]);
    return 0;
}

int dxv_render(dxv_ctx* c, const float eye[3], const float viewProj[16], const float posScale[4], uint32_t width,
               uint32_t height, uint8_t* rgbaHost)
{
    if (!c) return 1;
    Frame& f = cur_frame(c);
    const hipStream_t fs = cur_stream(c);
    if (!eye || !viewProj || !rgbaHost || !width || !height || width > 16384 || height > 16384)
        return fail(c, "dxv_render: bad arguments");
    if (!frame_renderable(f))
        return fail(c, "dxv_render: needs the whole grid of the last dxv_voxelize (z0 = 0, nz = grid_dim) on this context");
    const float unit[4] = {0.0f, 0.0f, 0.0f, 1.0f};                 // DXRVoxelizer.cpp:37
    RayCastCB cb;
    if (!update_frame(c->bound, posScale ? posScale : unit, eye, viewProj, (float)width, (float)height, cb))
        return fail(c, "dxv_render: singular view/projection chain");
    DXV_HIP(c, hipSetDevice(c->device));
    const size_t pixels = (size_t)width * height;
    DXV_HIP(c, c->image.reserve(pixels, pixels * 4, fs));
    if (dxv_sync(c)) return 1;                                       // the grid must be complete and valid
    // (the staging image is the context's: every frame's dxv_render ends in this host wait before another one can start)
    if (render_frame(c, cb, width, height, reinterpret_cast<uint8_t*>(c->image.p), (size_t)width * 4, true)) return 1;
    DXV_HIP(c, hipMemcpyAsync(rgbaHost, c->image.p, pixels * 4, hipMemcpyDeviceToHost, fs));
    DXV_HIP(c, hipStreamSynchronize(fs));
    timer_read(f.timers[kTimerRender]);
    return 0;
}

void* dxv_grid_device_ptr(dxv_ctx* c)
{
    if (!c) return nullptr;
    // the caller may write through the pointer now or at any later time (it stays valid until the grid is reallocated): from
    // here on every launch into this frame clears the grid itself instead of trusting what it wrote there last
    cur_frame(c).clearSig = 0;
    cur_frame(c).ptrExposed = true;
    return cur_frame(c).grid.p;
}
const void* dxv_grid_device_ptr_ro(const dxv_ctx* c) { return c ? c->frames[c->cur].grid.p : nullptr; }
size_t dxv_grid_bytes(const dxv_ctx* c) { return c ? c->frames[c->cur].gridBytes : 0; }

// the download and count entries: an unchecked launch of the selected frame is finished (with its redo, if any) first ...
static int finish_launch(dxv_ctx* c)
{
    if ((cur_frame(c).pending || cur_frame(c).grid_unsettled()) && dxv_sync(c)) return 1;     // (an edit in place whose verdict is not read yet: the grid may not be final)
    DXV_HIP(c, hipSetDevice(c->device));
    return 0;
}
// ... and the result comes back over the frame's stream, which is waited for
static int read_back(dxv_ctx* c, void* host, const void* src, size_t bytes)
{
    DXV_HIP(c, hipMemcpyAsync(host, src, bytes, hipMemcpyDeviceToHost, cur_stream(c)));
    DXV_HIP(c, hipStreamSynchronize(cur_stream(c)));
    return 0;
}

int dxv_grid_download(dxv_ctx* c, uint8_t* host, size_t bytes)
{
    if (!c) return 1;
    Frame& f = cur_frame(c);
    if (!host || bytes != f.gridBytes || !f.gridBytes) return fail(c, "dxv_grid_download: expected %zu bytes, got %zu", f.gridBytes, bytes);
    if (finish_launch(c)) return 1;
    return read_back(c, host, f.grid.p, bytes);
}

size_t dxv_grid_packed_bytes(const dxv_ctx* c) { return c ? (c->frames[c->cur].gridBytes + 7) / 8 : 0; }

int dxv_grid_download_packed(dxv_ctx* c, uint8_t* host, size_t bytes)
{
    if (!c) return 1;
    Frame& f = cur_frame(c);
    const size_t want = (f.gridBytes + 7) / 8;
    if (!host || !want || bytes != want) return fail(c, "dxv_grid_download_packed: expected %zu bytes, got %zu", want, bytes);
    if (finish_launch(c)) return 1;
    DXV_HIP(c, c->packed.reserve(want, align256(want), cur_stream(c)));
    DXV_HIP(c, launch_pack_bits(f.grid.p, f.gridBytes, c->packed.p, cur_stream(c)));
    return read_back(c, host, c->packed.p, want);
}

int dxv_grid_count(dxv_ctx* c, uint64_t* solid)
{
    if (!c) return 1;
    Frame& f = cur_frame(c);
    if (!solid || !f.gridBytes) return fail(c, "dxv_grid_count: no grid");
    if (finish_launch(c)) return 1;
    DXV_HIP(c, launch_count(f.grid.p, f.gridBytes, c->count.p, cur_stream(c)));
    unsigned long long v = 0;
    if (read_back(c, &v, c->count.p, sizeof(v))) return 1;
    *solid = v;
    return 0;
}

int dxv_enable_texels(dxv_ctx* c, int enable)
{
    if (!c) return 1;
    c->texels = enable != 0;
    return 0;
}

int dxv_texels_download(dxv_ctx* c, uint32_t* host, size_t bytes)
{
    if (!c) return 1;
    Frame& f = cur_frame(c);
    if (!c->texels || !f.texels.p) return fail(c, "dxv_texels_download: texel output not enabled");
    if (!host || bytes != f.gridBytes * 4) return fail(c, "dxv_texels_download: expected %zu bytes, got %zu", f.gridBytes * 4, bytes);
    if (finish_launch(c)) return 1;
    return read_back(c, host, f.texels.p, bytes);
}

int dxv_get_stats(const dxv_ctx* c, dxv_stats* out)
{
    if (!c || !out) return 1;
    *out = c->stats;
    const Frame& f = c->frames[c->cur];
    out->voxelize_ms = f.voxelize_ms; out->grid_dim = f.grid_dim; out->z0 = f.z0; out->nz = f.nz;
    out->stack_entries = f.stack_entries; out->redo_rays = f.redo_rays; out->row_block = f.row_block;
    out->list_entries = f.list_entries; out->list_res = f.list_res; out->list_ms = f.lastMode == DXV_MODE_PARITY ? c->rowLists.ms : c->lists.ms;
    out->plan_bricks = f.plan_bricks; out->plan_waves = f.plan_waves; out->plan_ms = f.plan_ms;
    out->plan_prepared = f.lastPrepared >= 0 ? 1u : 0u;
    out->render_ms = f.timers[kTimerRender].ms;
    return 0;
}

// dxv_policy.h holds the table: every key, the values it accepts, where its value lives.  Here: look up, check, store -- and the
// few keys whose setting does more than that.
int dxv_set_option(dxv_ctx* c, const char* key, int64_t value)
{
    if (!c || !key) return 1;
    const OptionRow* row = find_option(key);
    if (!row) return fail(c, "unknown option '%s'", key);
    if (!option_accepts(row->rule, value) || (row->effect == OptionEffect::brick && value >= num_brick_shapes()))
        return fail(c, "option %s: %lld %s", key, (long long)value, row->refusal);
    int& slot = c->opt.*row->where;
    switch (row->effect) {                                              // what has to happen in front of the store
    case OptionEffect::ablate:
#if !defined(DXV_ABLATE)
        // the timing-only variants of the lists kernel write wrong grids by design: they exist only in the library that
        // tools/ablate.py builds for itself (python -m dxrvoxelizer_amd.build --ablate -> libdxv_ablate.so)
        if (value != 0) return fail(c, "option ablate: this library was built without the ablation kernels (-DDXV_ABLATE)");
#endif
        break;
    case OptionEffect::plistres:
        if (slot != (int)value) { if (sync_frames(c)) return 1; c->rowLists.state = 0; }     // the next parity launch rebuilds the row lists
        break;
    case OptionEffect::listres:
        if (slot != (int)value && sync_frames(c)) return 1;             // the next launch rebuilds the lists: nothing may still read them
        break;
    case OptionEffect::lateralpad:
        // the lists are made with it: they go, with everything made of them (start table and start cells are rebuilt with them, the
        // prepared queues were probed against their mip, a counting pass dxv_refit left behind counted the other pad's records)
        if (slot != (int)value) {
            if (sync_frames(c) || settle_lists(c)) return 1;
            drop_prepared(c);
            c->lists.state = 0; c->specRes = 0;
            ++c->listEpoch;
        }
        break;
    default: break;
    }
    slot = (int)value;
    switch (row->effect) {                                              // ... and behind it
    case OptionEffect::wide:
        // the wide copy is a section of the scene: a scene built without it is built again
        if (value && c->haveScene && !c->hdr.hasWide) {
            if (!c->haveMesh) return fail(c, "option wide: this scene was imported without wide nodes; set the option on the exporting context before dxv_build");
            return dxv_build(c);
        }
        break;
    case OptionEffect::stack0:
        if (c->haveScene) c->stackNow = initial_stack(c);
        break;
    case OptionEffect::sortbits: radix_sort_set_plan((int)value); break;     // (the plan is the process's, not the context's)
    default: break;
    }
    return 0;
}

} // extern "C"
