// dxv_products.hip -- what is made of a frame's grid, and what edits it in place: distance field, mesh distance field, isosurface, octree and
// its expansion, components, their measures and select, fill, morph, thin -- the host side of each (the kernels: distance.hip, mesh_distance.hip,
// isosurface.hip, octree.hip, components.hip, measure.hip, thickness.hip, geodesic.hip, fill.hip, morph.hip, thin.hip), the accessors of what they made, and their halves of a frame's synchronisation.
#include "dxv_ctx.h"
#include "dxv_mesh_distance.h"
#include "dxv_fill.h"
#include "dxv_isosurface.h"
#include "dxv_octree.h"
#include "dxv_components.h"
#include "dxv_measure.h"
#include "dxv_morph.h"
#include "dxv_thin.h"
#include "dxv_thickness.h"
#include "dxv_geodesic.h"

using namespace dxv;
using namespace dxvhost;

namespace dxvhost {

// the refusals of whatever works on the whole grid of the selected frame
static int check_whole_grid(dxv_ctx* c, const char* who)
{
    const Frame& f = cur_frame(c);
    if (!f.grid.p || !f.grid_dim) return fail(c, "%s: frame %u has no grid yet (call dxv_voxelize first)", who, c->cur);
    if (!frame_renderable(f)) return fail(c, "%s: needs the whole grid of the frame's last launch (z0 = 0, nz = grid_dim), not a slab or a share", who);
    return 0;
}

// `want` bytes of something the selected frame holds and the caller has found current, into `host`, behind a synchronisation of the frame.
// (A NULL host is refused where there is something to copy: a current field has a side of at least 2 and a tree has its root, so only a mesh
// without vertices or a labelling without components gets as far as want == 0.)
static int download_current(dxv_ctx* c, const char* who, const void* src, size_t want, void* host, size_t bytes)
{
    if ((!host && want) || bytes != want) return fail(c, "%s: expected %zu bytes, got %zu", who, want, bytes);
    if (dxv_sync(c)) return 1;
    if (!want) return 0;
    DXV_HIP(c, hipMemcpyAsync(host, src, bytes, hipMemcpyDeviceToHost, cur_stream(c)));
    DXV_HIP(c, hipStreamSynchronize(cur_stream(c)));
    return 0;
}

// dxv_*_ms: the time the selected frame's last synchronisation read from one of its timers
static int timer_ms(dxv_ctx* c, const char* who, TimerUse use, float* ms)
{
    if (!c) return 1;
    if (!ms) return fail(c, "%s: ms is NULL", who);
    *ms = cur_frame(c).timers[use].ms;
    return 0;
}

// dxv_sync of one frame (sync_launch, once the stream has been waited for): the counters a select and a morph left in page-locked words
void read_products(dxv_ctx* c, uint32_t i)
{
    Frame& f = c->frames[i];
    if (f.selPending) {                                                 // the counters of the frame's last select (k_comp_keep has the LARGEST case)
        const unsigned long long* sel = c->pin->compSel[i];
        const bool largest = f.selRule == DXV_SELECT_LARGEST && f.selComponents;
        f.selKept = largest ? 1u : (uint32_t)sel[0];
        f.selDropped = largest ? f.selComponents - 1u : (uint32_t)sel[1];
        f.selChanged = largest ? sel[2] - (sel[3] >> 32) : sel[2];
        f.selPending = false;
    }
    if (f.morphPending) {                                               // the counters of the frame's last morph
        f.morphSet = c->pin->morphCount[i][0];
        f.morphCleared = c->pin->morphCount[i][1];
        f.morphPending = false;
    }
    if (f.thickPending) {                                               // the counters of the frame's last thickness
        f.thickCentres = c->pin->thickCount[i][0];
        f.thickItems = c->pin->thickCount[i][1];
        f.thickTested = c->pin->thickCount[i][2];
        f.thickSent = c->pin->thickCount[i][3];
        f.thickPending = false;
    }
}

// ... and the fill's half, behind it (the stream has been waited for): the verdict of the frame's last fill batch.  A batch whose last
// round still changed a word has not converged: further batches -- rounds and write-back, from the masks the frame's scratch still
// holds -- are enqueued and waited for until one has (the pattern of settle_lists: what only the host can decide is decided where the
// frame is synchronised anyway).  A flood over V voxels reaches at least one new voxel per live round: fewer than V rounds.
int settle_fill(dxv_ctx* c, uint32_t i)
{
    Frame& f = c->frames[i];
    const hipStream_t fs = frame_stream(c, i);
    const uint32_t* ctl = c->pin->fillCtl[i];
    Timer& t = f.timers[kTimerFill];
    const uint32_t N = f.grid_dim;
    const uint64_t most = f.fillBatch ? (uint64_t)N * N * N / f.fillBatch + 2u : 0u;
    for (uint64_t batch = 0; f.fillPending; ++batch) {
        uint32_t live = 0;
        while (live < f.fillBatch && ctl[live]) ++live;
        if (live < f.fillBatch) {                                       // round `live` changed nothing: the confirming round
            f.fillRounds += live + 1u;
            f.fillPending = false;
            break;
        }
        f.fillRounds += f.fillBatch;
        if (batch >= most) return fail(c, "dxv_fill: no fixed point after %u rounds on a grid of %u^3 voxels", f.fillRounds, N);
        DXV_HIP(c, launch_fill(f.grid.p, N, f.fillWhat, f.fillScratch.p, f.fillBatch, false, fs));
        if (t.armed) DXV_HIP(c, hipEventRecord(t.e1, fs));
        DXV_HIP(c, hipMemcpyAsync(c->pin->fillCtl[i], fill_control(f.fillScratch.p, N), sizeof(c->pin->fillCtl[i]), hipMemcpyDeviceToHost, fs));
        DXV_HIP(c, hipEventRecord(f.evEnd, fs));
        DXV_HIP(c, hipStreamSynchronize(fs));
    }
    timer_read(t);
    return 0;
}

// ... and the thin's, beside it (the stream has been waited for): the verdict of the frame's last thin batch, by the fill's discipline.  A batch all
// of whose iterations removed something has not reached the fixed point: unless max_iterations has been used up, a further batch -- iterations and
// write-back, from the masks the frame's scratch still holds -- is enqueued and waited for.  Every live iteration removes at least one of the
// V voxels: fewer than V iterations.
int settle_thin(dxv_ctx* c, uint32_t i)
{
    Frame& f = c->frames[i];
    const hipStream_t fs = frame_stream(c, i);
    const ThinControl& ctl = c->pin->thinCtl[i];
    Timer& t = f.timers[kTimerThin];
    const uint32_t N = f.grid_dim;
    const uint64_t most = f.thinBatch ? (uint64_t)N * N * N / f.thinBatch + 2u : 0u;
    for (uint64_t batch = 0; f.thinPending; ++batch) {
        uint32_t live = 0;
        while (live < f.thinInBatch && ctl.live[live]) ++live;
        f.thinRemoved = ctl.removed;
        if (live < f.thinInBatch) {                                     // iteration `live` removed nothing: the confirming iteration
            f.thinIterations += live + 1u;
            f.thinConverged = true;
            f.thinPending = false;
            break;
        }
        f.thinIterations += f.thinInBatch;
        if (f.thinBounded && !f.thinLeft) {                             // max_iterations stopped it first
            f.thinPending = false;
            break;
        }
        if (batch >= most) return fail(c, "dxv_thin: no fixed point after %u iterations on a grid of %u^3 voxels", f.thinIterations, N);
        f.thinInBatch = thin_batch(f.thinBatch, f.thinBounded ? f.thinLeft : 0u);
        if (f.thinBounded) f.thinLeft -= f.thinInBatch;
        DXV_HIP(c, launch_thin(f.grid.p, N, f.thinKind, f.thinScratch.p, f.thinInBatch, false, fs));
        if (t.armed) DXV_HIP(c, hipEventRecord(t.e1, fs));
        DXV_HIP(c, hipMemcpyAsync(&c->pin->thinCtl[i], f.thinScratch.p, sizeof(ThinControl), hipMemcpyDeviceToHost, fs));
        DXV_HIP(c, hipEventRecord(f.evEnd, fs));
        DXV_HIP(c, hipStreamSynchronize(fs));
    }
    timer_read(t);
    return 0;
}

// ... and the geodesic's (the stream has been waited for): the verdict of the frame's last geodesic batch, by the fill's discipline.  Word k of the
// control block is the number of live tiles of round k: a batch all of whose rounds had some has not reached the fixed point, and a further batch
// -- rounds from the flags the frame's scratch still holds, then the tally again -- is enqueued and waited for.  Every live round but the last
// lowers at least one word; the guard against a map that never settles is V rounds.
int settle_geodesic(dxv_ctx* c, uint32_t i)
{
    Frame& f = c->frames[i];
    const hipStream_t fs = frame_stream(c, i);
    const GeoControl& ctl = c->pin->geoCtl[i];
    Timer& t = f.timers[kTimerGeodesic];
    const uint32_t N = f.geoDim;
    const uint64_t most = f.geoBatch ? (uint64_t)N * N * N / f.geoBatch + 2u : 0u;
    for (uint64_t batch = 0; f.geoPending; ++batch) {
        uint32_t live = 0;
        while (live < f.geoBatch && ctl.live[live]) ++live;
        for (uint32_t k = 0; k < live; ++k) {                           // what the batch's live rounds ran (dxv_geodesic_work_info)
            f.geoTilesRun += ctl.live[k];
            if (ctl.live[k] > f.geoMostLive) f.geoMostLive = ctl.live[k];
            if (ctl.live[k] < kGeoSparseTiles) ++f.geoSparseRounds;
        }
        if (live < f.geoBatch) {                                        // round `live` found nothing live: the confirming round
            GeoTally tally{ctl.tally[0], ctl.tally[1], ctl.tally[2], ctl.tally[3]};
            f.geoRounds += live + 1u;
            f.geoSeedsUsed = tally.seeds; f.geoReached = tally.reached; f.geoUnreached = tally.unreached;
            f.geoFarthest = geo_tally_farthest(tally); f.geoFarthestVoxel = geo_tally_farthest_voxel(tally);
            f.geoPending = false;
            break;
        }
        f.geoRounds += f.geoBatch;
        if (batch >= most) return fail(c, "dxv_geodesic: no fixed point after %u rounds on a grid of %u^3 voxels", f.geoRounds, N);
        DXV_HIP(c, launch_geodesic_batch(f.geo.p, N, f.geoMetric, f.geoLimit, f.geoScratch.p, f.geoBatch, f.geoRounds, fs));
        if (t.armed) DXV_HIP(c, hipEventRecord(t.e1, fs));
        DXV_HIP(c, hipMemcpyAsync(&c->pin->geoCtl[i], f.geoScratch.p, sizeof(GeoControl), hipMemcpyDeviceToHost, fs));
        DXV_HIP(c, hipEventRecord(f.evEnd, fs));
        DXV_HIP(c, hipStreamSynchronize(fs));
    }
    timer_read(t);
    return 0;
}

// ... and the verdict of an expansion from a caller's tree (sync_launch has read the word): an index that could not be followed left empty
// voxels behind and is reported here, once
int settle_expand(dxv_ctx* c, uint32_t i)
{
    Frame& f = c->frames[i];
    if (!f.octExpandPending) return 0;
    f.octExpandPending = false;
    if (!c->pin->status[i][kOctStatusWord]) return 0;
    DXV_HIP(c, hipMemsetAsync(f.status.p + kOctStatusWord, 0, sizeof(uint32_t), frame_stream(c, i)));
    return fail(c, "dxv_octree_expand: the tree given for frame %u cannot be followed (a child index at or beyond its node count, or cells still mixed "
                   "after all its levels); the voxels behind such an index were left empty", i);
}

} // namespace dxvhost

extern "C" {

// The distance field of the selected frame's grid (distance.hip), enqueued on the frame's stream behind whatever it holds -- under
// dxv_render_async's host-wait rule, then the frame's end event behind it.  Field and scratch are the frame's own; growing them waits
// for that frame's stream only.
int dxv_distance_async(dxv_ctx* c, int format)
{
    if (!c) return 1;
    if (format != DXV_DIST_SQ_I32 && format != DXV_DIST_F32)
        return fail(c, "dxv_distance: unknown format %d (DXV_DIST_SQ_I32 = 0, DXV_DIST_F32 = 1)", format);
    if (check_whole_grid(c, "dxv_distance")) return 1;
    Frame& f = cur_frame(c);
    DXV_HIP(c, hipSetDevice(c->device));
    if (settle_frame_launch(c)) return 1;
    const hipStream_t fs = cur_stream(c);
    const uint32_t N = f.grid_dim;
    const size_t voxels = (size_t)N * N * N, scratch = distance_scratch_bytes(N);
    f.distVersion = 0; f.distDim = 0;
    DXV_HIP(c, f.dist.reserve(voxels, align256(voxels * sizeof(int32_t)), fs));
    DXV_HIP(c, f.distScratch.reserve(scratch, scratch, fs));
    const bool timed = c->opt.events != 0;
    DXV_HIP(c, timer_begin(f.timers[kTimerDistance], timed, fs));
    DXV_HIP(c, launch_distance(f.grid.p, N, format, f.dist.p, f.distScratch.p, fs));
    DXV_HIP(c, timer_end(f.timers[kTimerDistance], timed, fs));
    DXV_HIP(c, hipEventRecord(f.evEnd, fs));
    f.distDim = N; f.distFormat = format; f.distVersion = f.gridVersion;
    return 0;
}

int dxv_distance(dxv_ctx* c, int format)
{
    if (dxv_distance_async(c, format)) return 1;
    return dxv_sync(c);
}

// the frame's field, or the reason there is none to hand out: NULL + message
static const int32_t* current_field(const dxv_ctx* c, const char* who)
{
    const Frame& f = c->frames[c->cur];
    dxv_ctx* w = const_cast<dxv_ctx*>(c);                               // (the message is the one thing an accessor writes)
    if (!f.distDim || !f.dist.p) { (void)fail(w, "%s: frame %u has no distance field yet (call dxv_distance first)", who, c->cur); return nullptr; }
    if (f.distVersion != f.gridVersion) { (void)fail(w, "%s: frame %u was launched again since its distance field was made: the field is stale", who, c->cur); return nullptr; }
    return f.dist.p;
}

const void* dxv_distance_device_ptr(const dxv_ctx* c) { return c ? current_field(c, "dxv_distance_device_ptr") : nullptr; }

size_t dxv_distance_bytes(const dxv_ctx* c)
{
    if (!c) return 0;
    const Frame& f = c->frames[c->cur];
    return f.distVersion == f.gridVersion ? (size_t)f.distDim * f.distDim * f.distDim * sizeof(int32_t) : 0;
}

int dxv_distance_download(dxv_ctx* c, void* host, size_t bytes)
{
    if (!c) return 1;
    const int32_t* field = current_field(c, "dxv_distance_download");
    if (!field) return 1;
    return download_current(c, "dxv_distance_download", field, dxv_distance_bytes(c), host, bytes);
}

int dxv_distance_ms(dxv_ctx* c, float* ms) { return timer_ms(c, "dxv_distance_ms", kTimerDistance, ms); }

// The distance from the voxel centres of the selected frame's last launch to the MESH (mesh_distance.hip), signed by the frame's grid:
// enqueued on the frame's stream behind whatever it holds, under dxv_render_async's host-wait rule (a pending fill is settled by it),
// then the frame's end event; the frame is marked as reading the scene (sceneReadPending) until it is next synchronised, and dxv_refit and
// ensure_nodes make their stream wait for that event before they rewrite triangle records or node boxes.  Unlike the
// grid's own field a contiguous slab needs nothing from its neighbours; a share's slices are not one block of the field and are refused.
int dxv_mesh_distance_async(dxv_ctx* c, int format, uint32_t bandVoxels, int wantTriangles)
{
    if (!c) return 1;
    if (format != DXV_MDIST_VOXELS_F32 && format != DXV_MDIST_UNITS_F32)
        return fail(c, "dxv_mesh_distance: unknown format %d (DXV_MDIST_VOXELS_F32 = 0, DXV_MDIST_UNITS_F32 = 1)", format);
    if (bandVoxels > kMdMaxBand) return fail(c, "dxv_mesh_distance: a band of %u voxels (0 = none, at most %u)", bandVoxels, kMdMaxBand);
    Frame& f = cur_frame(c);
    if (!f.grid.p || !f.grid_dim || !f.nz) return fail(c, "dxv_mesh_distance: frame %u has no grid yet (call dxv_voxelize first)", c->cur);
    if (f.lastZBlock != f.nz)
        return fail(c, "dxv_mesh_distance: the frame's last launch was an interleaved share; needs the whole grid or a contiguous slab");
    if (!c->haveScene) return fail(c, "dxv_mesh_distance: no scene with a built hierarchy (call dxv_build or dxv_scene_import first)");
    if (c->hdr.treeHeight > (uint32_t)kMdStack)
        return fail(c, "dxv_mesh_distance: tree height %u exceeds the walk's column of %d entries", c->hdr.treeHeight, kMdStack);
    DXV_HIP(c, hipSetDevice(c->device));
    if (settle_frame_launch(c)) return 1;
    const hipStream_t fs = cur_stream(c);
    const bool walk = c->opt.mdistwalk != 0;
    if (walk && ensure_nodes(c, fs)) return 1;                          // after a refit that deferred the node boxes, as before a tree walk
    const uint32_t N = f.grid_dim;
    const size_t voxels = (size_t)N * N * f.nz;
    f.mdistVersion = 0; f.mdistDim = 0;
    DXV_HIP(c, f.mdist.reserve(voxels, align256(voxels * sizeof(float)), fs));
    if (wantTriangles) DXV_HIP(c, f.mdistTri.reserve(voxels, align256(voxels * sizeof(uint32_t)), fs));
    MeshDistanceParams p{};
    p.grid = f.grid.p; p.field = f.mdist.p; p.tris = wantTriangles ? f.mdistTri.p : nullptr;
    p.N = N; p.z0 = f.z0; p.nz = f.nz;
    p.format = format;
    p.cap = md_cap(N, bandVoxels);
    p.cullAbs = md_cull_abs(c->hdr.rootLo, c->hdr.rootHi);
    const bool timed = c->opt.events != 0;
    DXV_HIP(c, timer_begin(f.timers[kTimerMeshDistance], timed, fs));
    DXV_HIP(c, launch_mesh_distance(scene_nodes(c), scene_tripos(c), c->hdr.numTris, p, walk, fs));
    DXV_HIP(c, timer_end(f.timers[kTimerMeshDistance], timed, fs));
    DXV_HIP(c, hipEventRecord(f.evEnd, fs));
    f.sceneReadPending = true;
    f.mdistDim = N; f.mdistNz = f.nz; f.mdistFormat = format; f.mdistHasTri = wantTriangles != 0; f.mdistVersion = f.gridVersion;
    return 0;
}

int dxv_mesh_distance(dxv_ctx* c, int format, uint32_t bandVoxels, int wantTriangles)
{
    if (dxv_mesh_distance_async(c, format, bandVoxels, wantTriangles)) return 1;
    return dxv_sync(c);
}

// the frame's mesh distance field (triangles: its nearest triangles), or the reason there is none to hand out: NULL + message
static const void* current_mesh_field(const dxv_ctx* c, const char* who, bool triangles)
{
    const Frame& f = c->frames[c->cur];
    dxv_ctx* w = const_cast<dxv_ctx*>(c);                               // (the message is the one thing an accessor writes)
    if (!f.mdistDim || !f.mdist.p) { (void)fail(w, "%s: frame %u has no mesh distance field yet (call dxv_mesh_distance first)", who, c->cur); return nullptr; }
    if (f.mdistVersion != f.gridVersion) { (void)fail(w, "%s: frame %u was launched or filled again since its mesh distance field was made: the field is stale", who, c->cur); return nullptr; }
    if (triangles && !f.mdistHasTri) { (void)fail(w, "%s: frame %u's mesh distance field was made without triangles (want_triangles = 0)", who, c->cur); return nullptr; }
    return triangles ? static_cast<const void*>(f.mdistTri.p) : static_cast<const void*>(f.mdist.p);
}

const void* dxv_mesh_distance_device_ptr(const dxv_ctx* c) { return c ? current_mesh_field(c, "dxv_mesh_distance_device_ptr", false) : nullptr; }
const void* dxv_mesh_distance_triangles_device_ptr(const dxv_ctx* c) { return c ? current_mesh_field(c, "dxv_mesh_distance_triangles_device_ptr", true) : nullptr; }

size_t dxv_mesh_distance_bytes(const dxv_ctx* c)
{
    if (!c) return 0;
    const Frame& f = c->frames[c->cur];
    return f.mdistVersion == f.gridVersion ? (size_t)f.mdistDim * f.mdistDim * f.mdistNz * sizeof(float) : 0;
}

static int mesh_field_download(dxv_ctx* c, const char* who, bool triangles, void* host, size_t bytes)
{
    if (!c) return 1;
    const void* field = current_mesh_field(c, who, triangles);
    if (!field) return 1;
    return download_current(c, who, field, dxv_mesh_distance_bytes(c), host, bytes);
}
int dxv_mesh_distance_download(dxv_ctx* c, void* host, size_t bytes) { return mesh_field_download(c, "dxv_mesh_distance_download", false, host, bytes); }
int dxv_mesh_distance_triangles_download(dxv_ctx* c, void* host, size_t bytes) { return mesh_field_download(c, "dxv_mesh_distance_triangles_download", true, host, bytes); }

int dxv_mesh_distance_ms(dxv_ctx* c, float* ms) { return timer_ms(c, "dxv_mesh_distance_ms", kTimerMeshDistance, ms); }

// The isosurface of one of the selected frame's fields (isosurface.hip; dxv_isosurface.h has the rule), enqueued on the frame's stream behind
// whatever it holds, under dxv_render_async's host-wait rule: the count and scan kernels, the two totals into page-locked words and the
// one wait for them -- the pattern of dxv_prepare_launch's sixteen counts: the mesh's buffers cannot be sized without them --, then the emit
// kernel and the frame's end event, which nobody waits for here.
int dxv_isosurface_async(dxv_ctx* c, int source, float iso, int space)
{
    if (!c) return 1;
    if (source != DXV_ISO_MESH_DISTANCE && source != DXV_ISO_GRID_DISTANCE)
        return fail(c, "dxv_isosurface: unknown source %d (DXV_ISO_MESH_DISTANCE = 0, DXV_ISO_GRID_DISTANCE = 1)", source);
    if (space != DXV_ISO_SPACE_VOXELS && space != DXV_ISO_SPACE_OBJECT)
        return fail(c, "dxv_isosurface: unknown space %d (DXV_ISO_SPACE_VOXELS = 0, DXV_ISO_SPACE_OBJECT = 1)", space);
    if (!std::isfinite(iso)) return fail(c, "dxv_isosurface: iso must be finite, got %g", (double)iso);
    Frame& f = cur_frame(c);
    const float* field = nullptr;
    uint32_t N = 0;
    float P = 1.0f;
    if (source == DXV_ISO_MESH_DISTANCE) {
        if (!f.mdistDim || !f.mdist.p) return fail(c, "dxv_isosurface: frame %u has no mesh distance field yet (call dxv_mesh_distance first)", c->cur);
        if (f.mdistVersion != f.gridVersion) return fail(c, "dxv_isosurface: frame %u was launched or filled again since its mesh distance field was made: the field is stale", c->cur);
        if (f.mdistNz != f.mdistDim)
            return fail(c, "dxv_isosurface: the frame's mesh distance field is a slab's (%u of %u slices); needs the field of the whole grid", f.mdistNz, f.mdistDim);
        field = f.mdist.p; N = f.mdistDim;
        if (f.mdistFormat == DXV_MDIST_UNITS_F32) P = 2.0f / (float)N;
    } else {
        if (!f.distDim || !f.dist.p) return fail(c, "dxv_isosurface: frame %u has no distance field yet (call dxv_distance first)", c->cur);
        if (f.distVersion != f.gridVersion) return fail(c, "dxv_isosurface: frame %u was launched or filled again since its distance field was made: the field is stale", c->cur);
        if (f.distFormat != DXV_DIST_F32) return fail(c, "dxv_isosurface: the frame's distance field is in the int32 format; needs DXV_DIST_F32");
        field = reinterpret_cast<const float*>(f.dist.p); N = f.distDim;
    }
    if (space == DXV_ISO_SPACE_OBJECT && !c->haveScene)
        return fail(c, "dxv_isosurface: DXV_ISO_SPACE_OBJECT needs the scene's bound and the context has no scene (call dxv_build or dxv_scene_import, or ask for DXV_ISO_SPACE_VOXELS)");
    DXV_HIP(c, hipSetDevice(c->device));
    if (settle_frame_launch(c)) return 1;
    const hipStream_t fs = cur_stream(c);
    const size_t scratch = iso_scratch_bytes(N);
    DXV_HIP(c, f.isoScratch.reserve(scratch, scratch, fs));
    IsoParams p{};
    p.field = field; p.N = N; p.iso = iso; p.P = P; p.object = space == DXV_ISO_SPACE_OBJECT;
    memcpy(p.bound, c->bound, sizeof(p.bound));
    iso_scratch_layout(f.isoScratch.p, N, p);
    const bool timed = c->opt.events != 0;
    unsigned long long* totals = c->pin->isoTotals[c->cur];
    DXV_HIP(c, timer_begin(f.timers[kTimerIso], timed, fs));
    DXV_HIP(c, launch_iso_count(p, fs));
    DXV_HIP(c, hipMemcpyAsync(totals, p.totals, 2 * sizeof(unsigned long long), hipMemcpyDeviceToHost, fs));
    DXV_HIP(c, hipStreamSynchronize(fs));
    const unsigned long long vertices = totals[0], quads = totals[1];
    if (vertices > kIsoMaxCount || quads > kIsoMaxCount / 6u)
        return fail(c, "dxv_isosurface: a mesh of %llu vertices and %llu index words; at most %llu of each (the frame's earlier mesh is kept)", vertices,
                    6u * quads, (unsigned long long)kIsoMaxCount);
    f.isoVersion = 0;
    if (vertices) {
        DXV_HIP(c, f.isoVb.reserve((size_t)vertices, align256((size_t)vertices * sizeof(IsoVertex)), fs));
        if (quads) DXV_HIP(c, f.isoIb.reserve(6 * (size_t)quads, align256(6 * (size_t)quads * sizeof(uint32_t)), fs));
        p.vb = reinterpret_cast<IsoVertex*>(f.isoVb.p); p.ib = f.isoIb.p;
        DXV_HIP(c, launch_iso_emit(p, fs));
    }
    DXV_HIP(c, timer_end(f.timers[kTimerIso], timed, fs));
    DXV_HIP(c, hipEventRecord(f.evEnd, fs));
    f.isoVertices = (uint32_t)vertices; f.isoTriangles = (uint32_t)(2u * quads);
    f.isoHave = true; f.isoVersion = f.gridVersion;
    return 0;
}

int dxv_isosurface(dxv_ctx* c, int source, float iso, int space)
{
    if (dxv_isosurface_async(c, source, iso, space)) return 1;
    return dxv_sync(c);
}

// whether the frame has a mesh to hand out: 0, or 1 with the reason as the message
static int current_mesh(const dxv_ctx* c, const char* who)
{
    const Frame& f = c->frames[c->cur];
    dxv_ctx* w = const_cast<dxv_ctx*>(c);                               // (the message is the one thing an accessor writes)
    if (!f.isoHave) return fail(w, "%s: frame %u has no isosurface yet (call dxv_isosurface first)", who, c->cur);
    if (f.isoVersion != f.gridVersion) return fail(w, "%s: frame %u was launched or filled again since its isosurface was made: the mesh is stale", who, c->cur);
    return 0;
}

int dxv_isosurface_counts(dxv_ctx* c, uint32_t* vertices, uint32_t* triangles)
{
    if (!c) return 1;
    if (current_mesh(c, "dxv_isosurface_counts")) return 1;
    if (vertices) *vertices = cur_frame(c).isoVertices;
    if (triangles) *triangles = cur_frame(c).isoTriangles;
    return 0;
}

const void* dxv_isosurface_vertices_device_ptr(const dxv_ctx* c)
{
    if (!c || current_mesh(c, "dxv_isosurface_vertices_device_ptr")) return nullptr;
    return c->frames[c->cur].isoVertices ? c->frames[c->cur].isoVb.p : nullptr;
}
const void* dxv_isosurface_indices_device_ptr(const dxv_ctx* c)
{
    if (!c || current_mesh(c, "dxv_isosurface_indices_device_ptr")) return nullptr;
    return c->frames[c->cur].isoTriangles ? c->frames[c->cur].isoIb.p : nullptr;
}

int dxv_isosurface_vertices_download(dxv_ctx* c, void* host, size_t bytes)
{
    if (!c || current_mesh(c, "dxv_isosurface_vertices_download")) return 1;
    return download_current(c, "dxv_isosurface_vertices_download", cur_frame(c).isoVb.p, (size_t)cur_frame(c).isoVertices * sizeof(IsoVertex), host, bytes);
}
int dxv_isosurface_indices_download(dxv_ctx* c, void* host, size_t bytes)
{
    if (!c || current_mesh(c, "dxv_isosurface_indices_download")) return 1;
    return download_current(c, "dxv_isosurface_indices_download", cur_frame(c).isoIb.p, (size_t)cur_frame(c).isoTriangles * 3u * sizeof(uint32_t), host, bytes);
}

int dxv_isosurface_ms(dxv_ctx* c, float* ms) { return timer_ms(c, "dxv_isosurface_ms", kTimerIso, ms); }

// The sparse voxel octree of the selected frame's grid (octree.hip; dxv_octree.h has the rule), enqueued on the frame's stream behind whatever
// it holds, under dxv_render_async's host-wait rule: the reduce and scan kernels, the L + 1 level totals into page-locked words and the one
// wait for them -- the pattern of dxv_isosurface_async: the node buffer cannot be sized without the last of them --, then the emit kernel and
// the frame's end event, which nobody waits for here.
int dxv_octree_async(dxv_ctx* c)
{
    if (!c) return 1;
    if (check_whole_grid(c, "dxv_octree")) return 1;
    Frame& f = cur_frame(c);
    DXV_HIP(c, hipSetDevice(c->device));
    if (settle_frame_launch(c)) return 1;
    const hipStream_t fs = cur_stream(c);
    const uint32_t N = f.grid_dim;
    const size_t scratch = oct_scratch_bytes(N);
    DXV_HIP(c, f.octScratch.reserve(scratch, scratch, fs));
    OctParams p{};
    p.grid = f.grid.p;
    oct_scratch_layout(f.octScratch.p, N, p);
    const uint32_t L = p.L;
    const bool timed = c->opt.events != 0;
    unsigned long long* totals = c->pin->octTotals[c->cur];
    DXV_HIP(c, timer_begin(f.timers[kTimerOctree], timed, fs));
    DXV_HIP(c, launch_oct_count(p, fs));
    DXV_HIP(c, hipMemcpyAsync(totals, p.levelFirst, (L + 1u) * sizeof(unsigned long long), hipMemcpyDeviceToHost, fs));
    DXV_HIP(c, hipStreamSynchronize(fs));
    const unsigned long long nodes = totals[L];
    if (!nodes || nodes > kOctMaxNodes)
        return fail(c, "dxv_octree: a tree of %llu nodes; at least the root and at most %llu (the frame's earlier tree is kept)", nodes,
                    (unsigned long long)kOctMaxNodes);
    f.octVersion = 0;
    DXV_HIP(c, f.octNodes.reserve((size_t)nodes, align256((size_t)nodes * 2u * sizeof(uint32_t)), fs));
    p.nodes = f.octNodes.p;
    DXV_HIP(c, launch_oct_emit(p, fs));
    DXV_HIP(c, timer_end(f.timers[kTimerOctree], timed, fs));
    DXV_HIP(c, hipEventRecord(f.evEnd, fs));
    f.octLevels = L; f.octCount = (uint32_t)nodes;
    for (uint32_t l = 0; l < 12u; ++l) f.octLevelFirst[l] = l <= L ? (uint32_t)totals[l] : 0u;
    f.octHave = true; f.octVersion = f.gridVersion;
    return 0;
}

int dxv_octree(dxv_ctx* c)
{
    if (dxv_octree_async(c)) return 1;
    return dxv_sync(c);
}

// whether the frame has a tree to hand out: 0, or 1 with the reason as the message
static int current_tree(const dxv_ctx* c, const char* who)
{
    const Frame& f = c->frames[c->cur];
    dxv_ctx* w = const_cast<dxv_ctx*>(c);                               // (the message is the one thing an accessor writes)
    if (!f.octHave) return fail(w, "%s: frame %u has no octree yet (call dxv_octree first)", who, c->cur);
    if (f.octVersion != f.gridVersion) return fail(w, "%s: frame %u was launched, filled or expanded again since its octree was made: the tree is stale", who, c->cur);
    return 0;
}

int dxv_octree_info(dxv_ctx* c, uint32_t* levels, uint32_t* nodes, uint32_t level_first[12])
{
    if (!c) return 1;
    if (current_tree(c, "dxv_octree_info")) return 1;
    const Frame& f = cur_frame(c);
    if (levels) *levels = f.octLevels;
    if (nodes) *nodes = f.octCount;
    if (level_first) memcpy(level_first, f.octLevelFirst, sizeof(f.octLevelFirst));
    return 0;
}

const void* dxv_octree_device_ptr(const dxv_ctx* c)
{
    if (!c || current_tree(c, "dxv_octree_device_ptr")) return nullptr;
    return c->frames[c->cur].octNodes.p;
}

size_t dxv_octree_bytes(const dxv_ctx* c)
{
    if (!c) return 0;
    const Frame& f = c->frames[c->cur];
    return f.octHave && f.octVersion == f.gridVersion ? (size_t)f.octCount * 2u * sizeof(uint32_t) : 0;
}

int dxv_octree_download(dxv_ctx* c, void* host, size_t bytes)
{
    if (!c || current_tree(c, "dxv_octree_download")) return 1;
    return download_current(c, "dxv_octree_download", cur_frame(c).octNodes.p, dxv_octree_bytes(c), host, bytes);
}

int dxv_octree_ms(dxv_ctx* c, float* ms) { return timer_ms(c, "dxv_octree_ms", kTimerOctree, ms); }

// The selected frame's grid from an octree (octree.hip: k_oct_expand), in place, enqueued on the frame's stream behind whatever it holds --
// under dxv_render_async's host-wait rule and dxv_fill_async's rules for the grid.  A caller's tree is not trusted: the kernel compares every
// index with `nodes` before it follows it, and what it had to refuse is read where the frame is next synchronised (settle_expand).
int dxv_octree_expand_async(dxv_ctx* c, const void* deviceNodes, uint32_t nodes, uint32_t levels)
{
    if (!c) return 1;
    if (check_whole_grid(c, "dxv_octree_expand")) return 1;
    Frame& f = cur_frame(c);
    const uint32_t N = f.grid_dim, L = oct_levels(N);
    DXV_HIP(c, hipSetDevice(c->device));
    const bool own = deviceNodes == nullptr;
    if (own) {
        if (current_tree(c, "dxv_octree_expand")) return 1;
        deviceNodes = f.octNodes.p; nodes = f.octCount;                 // (a current tree is the tree of this grid: its levels are L)
    } else {
        if (!nodes) return fail(c, "dxv_octree_expand: a tree of 0 nodes (the root is always there: nodes >= 1)");
        if (nodes > kOctMaxNodes) return fail(c, "dxv_octree_expand: a tree of %u nodes; at most %llu", nodes, (unsigned long long)kOctMaxNodes);
        if (levels != L) return fail(c, "dxv_octree_expand: a tree of %u levels; the frame's grid of %u^3 voxels has %u", levels, N, L);
        if (reinterpret_cast<uintptr_t>(deviceNodes) % 4) return fail(c, "dxv_octree_expand: nodes at %p: need a 4-byte aligned pointer", deviceNodes);
        const size_t need = (size_t)nodes * 2u * sizeof(uint32_t);
        size_t room = 0;
        if (const int r = check_device_range(c, "dxv_octree_expand", deviceNodes, need, &room))
            return r == 1 ? 1 : fail(c, "dxv_octree_expand: %u nodes need %zu bytes, the allocation behind %p has %zu", nodes, need, deviceNodes, room);
    }
    if (settle_frame_launch(c)) return 1;
    const hipStream_t fs = cur_stream(c);
    // the grid stops being what the frame's last launch wrote (dxv_fill_async's rules): a kept queue's zeros are gone, and whatever was made
    // of the grid before -- fields, the mesh, the frame's own tree -- is stale
    f.clearSig = 0;
    grid_rewritten(f);
    DXV_HIP(c, launch_oct_expand(f.grid.p, N, static_cast<const uint32_t*>(deviceNodes), nodes, f.status.p + kOctStatusWord, fs));
    DXV_HIP(c, hipEventRecord(f.evEnd, fs));
    if (!own) f.octExpandPending = true;                                // (the frame's own tree was made by the build: it has nothing to report)
    return 0;
}

int dxv_octree_expand(dxv_ctx* c, const void* deviceNodes, uint32_t nodes, uint32_t levels)
{
    if (dxv_octree_expand_async(c, deviceNodes, nodes, levels)) return 1;
    return dxv_sync(c);
}

// The connected components of the selected frame's grid (components.hip; dxv_components.h has the rule's routines), enqueued on the frame's
// stream behind whatever it holds, under dxv_render_async's host-wait rule: pack, init, merge, compress and the numbering, K into a
// page-locked word and the one wait for it -- the pattern of dxv_octree_async: the table cannot be sized without it --, then the stats kernels
// and the frame's end event, which nobody waits for here.
int dxv_components_async(dxv_ctx* c, int of, int connectivity)
{
    if (!c) return 1;
    if (of != DXV_COMP_SOLID && of != DXV_COMP_EMPTY) return fail(c, "dxv_components: unknown kind %d (DXV_COMP_SOLID = 0, DXV_COMP_EMPTY = 1)", of);
    if (connectivity != 6 && connectivity != 26) return fail(c, "dxv_components: connectivity %d (6 or 26)", connectivity);
    if (check_whole_grid(c, "dxv_components")) return 1;
    Frame& f = cur_frame(c);
    const uint32_t N = f.grid_dim;
    if (N > kCompMaxN) return fail(c, "dxv_components: a grid of %u^3 voxels; at most %u^3 (a label and a linear index must fit 32 bits)", N, kCompMaxN);
    DXV_HIP(c, hipSetDevice(c->device));
    if (settle_frame_launch(c)) return 1;
    const hipStream_t fs = cur_stream(c);
    const size_t voxels = (size_t)N * N * N, scratch = comp_scratch_bytes(N);
    DXV_HIP(c, f.compScratch.reserve(scratch, scratch, fs));
    f.compVersion = 0;                                                  // (the build writes into the frame's label buffer: what it held is gone)
    f.measVersion = 0;                                                  // (... and a measure of the labels it held with it)
    DXV_HIP(c, f.compLabels.reserve(voxels, align256(voxels * sizeof(uint32_t)), fs));
    CompParams p{};
    p.grid = f.grid.p; p.of = of; p.connectivity = (uint32_t)connectivity; p.labels = f.compLabels.p;
    comp_scratch_layout(f.compScratch.p, N, p);
    const bool timed = c->opt.events != 0;
    unsigned long long* total = &c->pin->compTotal[c->cur];
    DXV_HIP(c, timer_begin(f.timers[kTimerComponents], timed, fs));
    DXV_HIP(c, launch_comp_label(p, fs));
    DXV_HIP(c, hipMemcpyAsync(total, p.total, sizeof(unsigned long long), hipMemcpyDeviceToHost, fs));
    DXV_HIP(c, hipStreamSynchronize(fs));
    const uint32_t K = (uint32_t)*total;
    if (K) {
        DXV_HIP(c, f.compTable.reserve(K, align256((size_t)K * sizeof(CompRecord)), fs));
        DXV_HIP(c, f.compWork.reserve((size_t)K * sizeof(CompStats), align256((size_t)K * sizeof(CompStats)), fs));
        p.table = reinterpret_cast<CompRecord*>(f.compTable.p);
        p.stats = reinterpret_cast<CompStats*>(f.compWork.p);
        DXV_HIP(c, launch_comp_stats(p, K, fs));
    }
    DXV_HIP(c, timer_end(f.timers[kTimerComponents], timed, fs));
    DXV_HIP(c, hipEventRecord(f.evEnd, fs));
    f.compCount = K; f.compDim = N; f.compOf = of; f.compConnectivity = connectivity;
    f.compHave = true; f.compVersion = f.gridVersion;
    return 0;
}

int dxv_components(dxv_ctx* c, int of, int connectivity)
{
    if (dxv_components_async(c, of, connectivity)) return 1;
    return dxv_sync(c);
}

// whether the frame has labels to hand out: 0, or 1 with the reason as the message
static int current_labels(const dxv_ctx* c, const char* who)
{
    const Frame& f = c->frames[c->cur];
    dxv_ctx* w = const_cast<dxv_ctx*>(c);                               // (the message is the one thing an accessor writes)
    if (!f.compHave) return fail(w, "%s: frame %u has no components yet (call dxv_components first)", who, c->cur);
    if (f.compVersion != f.gridVersion)
        return fail(w, "%s: frame %u was launched, filled, expanded or selected again since its components were labelled: labels and table are stale", who, c->cur);
    return 0;
}

int dxv_components_info(dxv_ctx* c, uint32_t* count, int* of, int* connectivity)
{
    if (!c) return 1;
    if (current_labels(c, "dxv_components_info")) return 1;
    const Frame& f = cur_frame(c);
    if (count) *count = f.compCount;
    if (of) *of = f.compOf;
    if (connectivity) *connectivity = f.compConnectivity;
    return 0;
}

const void* dxv_components_labels_device_ptr(const dxv_ctx* c)
{
    if (!c || current_labels(c, "dxv_components_labels_device_ptr")) return nullptr;
    return c->frames[c->cur].compLabels.p;
}
size_t dxv_components_labels_bytes(const dxv_ctx* c)
{
    if (!c) return 0;
    const Frame& f = c->frames[c->cur];
    return f.compHave && f.compVersion == f.gridVersion ? (size_t)f.compDim * f.compDim * f.compDim * sizeof(uint32_t) : 0;
}
const void* dxv_components_table_device_ptr(const dxv_ctx* c)
{
    if (!c || current_labels(c, "dxv_components_table_device_ptr")) return nullptr;
    return c->frames[c->cur].compCount ? c->frames[c->cur].compTable.p : nullptr;
}
size_t dxv_components_table_bytes(const dxv_ctx* c)
{
    if (!c) return 0;
    const Frame& f = c->frames[c->cur];
    return f.compHave && f.compVersion == f.gridVersion ? (size_t)f.compCount * sizeof(CompRecord) : 0;
}

int dxv_components_labels_download(dxv_ctx* c, void* host, size_t bytes)
{
    if (!c || current_labels(c, "dxv_components_labels_download")) return 1;
    return download_current(c, "dxv_components_labels_download", cur_frame(c).compLabels.p, dxv_components_labels_bytes(c), host, bytes);
}
int dxv_components_table_download(dxv_ctx* c, void* host, size_t bytes)
{
    if (!c || current_labels(c, "dxv_components_table_download")) return 1;
    return download_current(c, "dxv_components_table_download", cur_frame(c).compTable.p, dxv_components_table_bytes(c), host, bytes);
}

int dxv_components_ms(dxv_ctx* c, float* ms) { return timer_ms(c, "dxv_components_ms", kTimerComponents, ms); }

// The integral measures of the selected frame's current labelling (measure.hip; dxv_measure.h has the rule's routines), enqueued on the frame's
// stream behind whatever it holds, under dxv_render_async's host-wait rule.  K is known from the labelling: nothing is read back.  The member
// mask is the labelling's own; once dxv_trim has released it, it is packed again from the grid, which a current labelling guarantees unchanged.
int dxv_measure_async(dxv_ctx* c)
{
    if (!c) return 1;
    if (check_whole_grid(c, "dxv_measure")) return 1;
    if (current_labels(c, "dxv_measure")) return 1;
    Frame& f = cur_frame(c);
    if (f.grid_dim != f.compDim) return fail(c, "dxv_measure: the labels of frame %u do not belong to its grid: they are stale", c->cur);
    DXV_HIP(c, hipSetDevice(c->device));
    if (settle_frame_launch(c)) return 1;
    const hipStream_t fs = cur_stream(c);
    const uint32_t N = f.compDim, K = f.compCount;
    const bool packed = f.compScratch.p != nullptr;                     // (the mask of the frame's last labelling: this one, it is current)
    const size_t scratch = comp_scratch_bytes(N);
    DXV_HIP(c, f.compScratch.reserve(scratch, scratch, fs));
    f.measVersion = 0;
    DXV_HIP(c, f.measTable.reserve((size_t)K + 1u, align256(measure_table_bytes(K)), fs));
    CompParams p{};
    comp_scratch_layout(f.compScratch.p, N, p);
    const bool timed = c->opt.events != 0;
    DXV_HIP(c, timer_begin(f.timers[kTimerMeasure], timed, fs));
    if (!packed) DXV_HIP(c, launch_comp_pack(f.grid.p, N, f.compOf, p.mask, fs));
    DXV_HIP(c, launch_measure(p.mask, N, (uint32_t)f.compConnectivity, f.compLabels.p, K, f.measTable.p, fs));
    DXV_HIP(c, timer_end(f.timers[kTimerMeasure], timed, fs));
    DXV_HIP(c, hipEventRecord(f.evEnd, fs));
    f.measCount = K; f.measHave = true; f.measVersion = f.gridVersion;
    return 0;
}

int dxv_measure(dxv_ctx* c)
{
    if (dxv_measure_async(c)) return 1;
    return dxv_sync(c);
}

// whether the frame has a measure to hand out: 0, or 1 with the reason as the message
static int current_measure(const dxv_ctx* c, const char* who)
{
    const Frame& f = c->frames[c->cur];
    dxv_ctx* w = const_cast<dxv_ctx*>(c);                               // (the message is the one thing an accessor writes)
    if (!f.measHave) return fail(w, "%s: frame %u has no measure yet (call dxv_measure first)", who, c->cur);
    if (f.measVersion != f.gridVersion || f.compVersion != f.gridVersion)
        return fail(w, "%s: frame %u was launched, edited or labelled again since its components were measured: the measure is stale", who, c->cur);
    return 0;
}

const void* dxv_measure_table_device_ptr(const dxv_ctx* c)
{
    if (!c || current_measure(c, "dxv_measure_table_device_ptr")) return nullptr;
    return c->frames[c->cur].measTable.p;
}
size_t dxv_measure_table_bytes(const dxv_ctx* c)
{
    if (!c || current_measure(c, "dxv_measure_table_bytes")) return 0;
    return measure_table_bytes(c->frames[c->cur].measCount);
}
int dxv_measure_table_download(dxv_ctx* c, void* host, size_t bytes)
{
    if (!c || current_measure(c, "dxv_measure_table_download")) return 1;
    return download_current(c, "dxv_measure_table_download", cur_frame(c).measTable.p, dxv_measure_table_bytes(c), host, bytes);
}

int dxv_measure_ms(dxv_ctx* c, float* ms) { return timer_ms(c, "dxv_measure_ms", kTimerMeasure, ms); }

// The local thickness of the selected frame's grid (thickness.hip; dxv_thickness.h has the rule's routines), enqueued on the frame's stream behind
// whatever it holds, under dxv_render_async's host-wait rule.  A fixed chain of kernels that read their counts from device memory: nothing is
// read back, the four counters go into page-locked words and are read where the frame is next synchronised.  Map, histogram and scratch are the
// frame's own; the field of the grid is made into the scratch, never into the frame's distance field.
int dxv_thickness_async(dxv_ctx* c, int of, uint32_t cap_sq)
{
    if (!c) return 1;
    if (of != DXV_COMP_SOLID && of != DXV_COMP_EMPTY) return fail(c, "dxv_thickness: unknown kind %d (DXV_COMP_SOLID = 0, DXV_COMP_EMPTY = 1)", of);
    if (cap_sq < kThickMinCapSq || cap_sq > kThickMaxCapSq) return fail(c, "dxv_thickness: cap_sq %u is not in [%u, %u]", cap_sq, kThickMinCapSq, kThickMaxCapSq);
    if (check_whole_grid(c, "dxv_thickness")) return 1;
    Frame& f = cur_frame(c);
    const uint32_t N = f.grid_dim;
    if (N > kThickMaxN) return fail(c, "dxv_thickness: a grid of %u^3 voxels; at most %u^3 (a centre's linear index must fit 30 bits)", N, kThickMaxN);
    DXV_HIP(c, hipSetDevice(c->device));
    if (settle_frame_launch(c)) return 1;
    const hipStream_t fs = cur_stream(c);
    const size_t voxels = (size_t)N * N * N, scratch = thickness_scratch_bytes(N);
    f.thickVersion = 0; f.thickDim = 0;
    DXV_HIP(c, f.thick.reserve(voxels, align256(voxels * sizeof(uint32_t)), fs));
    DXV_HIP(c, f.thickHist.reserve(kThickMaxCapSq + 1u, align256(thickness_histogram_bytes(kThickMaxCapSq)), fs));
    DXV_HIP(c, f.thickScratch.reserve(scratch, scratch, fs));
    ThickParams p{};
    p.of = of; p.cap = cap_sq; p.cull = (uint32_t)c->opt.thickcull; p.count = c->opt.thickstages ? 1u : 0u; p.W = f.thick.p; p.hist = f.thickHist.p;
    thickness_layout(f.thickScratch.p, N, p);
    const bool timed = c->opt.events != 0, staged = timed && c->opt.thickstages != 0;      // (the stages' own pairs only for a caller that measures)
    DXV_HIP(c, timer_begin(f.timers[kTimerThickness], timed, fs));
    for (int stage = 0; stage < THICK_STAGES; ++stage) {
        Timer& t = f.timers[kTimerThickStage0 + stage];
        if (!staged) t.ms = 0.0f;
        DXV_HIP(c, timer_begin(t, staged, fs));
        DXV_HIP(c, launch_thickness_stage(f.grid.p, p, stage, fs));
        DXV_HIP(c, timer_end(t, staged, fs));
    }
    DXV_HIP(c, timer_end(f.timers[kTimerThickness], timed, fs));
    DXV_HIP(c, hipMemcpyAsync(c->pin->thickCount[c->cur], thickness_counters(p), sizeof(c->pin->thickCount[c->cur]), hipMemcpyDeviceToHost, fs));
    DXV_HIP(c, hipEventRecord(f.evEnd, fs));
    f.thickPending = true;
    f.thickDim = N; f.thickCap = cap_sq; f.thickVersion = f.gridVersion;
    return 0;
}

int dxv_thickness(dxv_ctx* c, int of, uint32_t cap_sq)
{
    if (dxv_thickness_async(c, of, cap_sq)) return 1;
    return dxv_sync(c);
}

// whether the frame has a thickness map to hand out: 0, or 1 with the reason as the message
static int current_thickness(const dxv_ctx* c, const char* who)
{
    const Frame& f = c->frames[c->cur];
    dxv_ctx* w = const_cast<dxv_ctx*>(c);                               // (the message is the one thing an accessor writes)
    if (!f.thickDim || !f.thick.p) return fail(w, "%s: frame %u has no thickness map yet (call dxv_thickness first)", who, c->cur);
    if (f.thickVersion != f.gridVersion)
        return fail(w, "%s: frame %u was launched or edited again since its thickness map was made: map and histogram are stale", who, c->cur);
    return 0;
}

const void* dxv_thickness_device_ptr(const dxv_ctx* c)
{
    if (!c || current_thickness(c, "dxv_thickness_device_ptr")) return nullptr;
    return c->frames[c->cur].thick.p;
}
size_t dxv_thickness_bytes(const dxv_ctx* c)
{
    if (!c) return 0;
    const Frame& f = c->frames[c->cur];
    return f.thickDim && f.thickVersion == f.gridVersion ? (size_t)f.thickDim * f.thickDim * f.thickDim * sizeof(uint32_t) : 0;
}
int dxv_thickness_download(dxv_ctx* c, void* host, size_t bytes)
{
    if (!c || current_thickness(c, "dxv_thickness_download")) return 1;
    return download_current(c, "dxv_thickness_download", cur_frame(c).thick.p, dxv_thickness_bytes(c), host, bytes);
}
size_t dxv_thickness_histogram_bytes(const dxv_ctx* c)
{
    if (!c) return 0;
    const Frame& f = c->frames[c->cur];
    return f.thickDim && f.thickVersion == f.gridVersion ? thickness_histogram_bytes(f.thickCap) : 0;
}
int dxv_thickness_histogram_download(dxv_ctx* c, void* host, size_t bytes)
{
    if (!c || current_thickness(c, "dxv_thickness_histogram_download")) return 1;
    return download_current(c, "dxv_thickness_histogram_download", cur_frame(c).thickHist.p, dxv_thickness_histogram_bytes(c), host, bytes);
}

int dxv_thickness_info(dxv_ctx* c, float* ms, uint64_t* centres_painted, uint64_t* work_items)
{
    if (!c) return 1;
    const Frame& f = cur_frame(c);
    if (ms) *ms = f.timers[kTimerThickness].ms;
    if (centres_painted) *centres_painted = f.thickCentres;
    if (work_items) *work_items = f.thickItems;
    return 0;
}

int dxv_thickness_stage_info(dxv_ctx* c, float ms[6], uint64_t* voxels_tested, uint64_t* atomics_sent)
{
    if (!c) return 1;
    if (!ms) return fail(c, "dxv_thickness_stage_info: ms is NULL");
    const Frame& f = cur_frame(c);
    for (int stage = 0; stage < THICK_STAGES; ++stage) ms[stage] = f.timers[kTimerThickStage0 + stage].ms;
    if (voxels_tested) *voxels_tested = f.thickTested;
    if (atomics_sent) *atomics_sent = f.thickSent;
    return 0;
}

// The geodesic distance inside the selected frame's grid (geodesic.hip; dxv_geodesic.h has the rule's routines), enqueued on the frame's stream
// behind whatever it holds, under dxv_render_async's host-wait rule and the fill's discipline: the init, ONE batch of rounds, the tally, the
// batch's control block into page-locked words, the frame's end event.  Whether the batch reached the fixed point is read where the frame is
// next synchronised (settle_geodesic).  Everything is refused before anything is enqueued or allocated; the grid is only read.
int dxv_geodesic_async(dxv_ctx* c, int of, int metric, int seeds_kind, const void* seeds, uint32_t seed_count, uint32_t limit)
{
    if (!c) return 1;
    if (of != DXV_COMP_SOLID && of != DXV_COMP_EMPTY) return fail(c, "dxv_geodesic: unknown kind %d (DXV_COMP_SOLID = 0, DXV_COMP_EMPTY = 1)", of);
    if (metric != DXV_GEO_FACES && metric != DXV_GEO_CHAMFER) return fail(c, "dxv_geodesic: unknown metric %d (DXV_GEO_FACES = 0, DXV_GEO_CHAMFER = 1)", metric);
    if (seeds_kind != DXV_GEO_SEEDS_BORDER && seeds_kind != DXV_GEO_SEEDS_LIST && seeds_kind != DXV_GEO_SEEDS_MASK)
        return fail(c, "dxv_geodesic: unknown seed kind %d (DXV_GEO_SEEDS_BORDER = 0, DXV_GEO_SEEDS_LIST = 1, DXV_GEO_SEEDS_MASK = 2)", seeds_kind);
    if (seeds_kind == DXV_GEO_SEEDS_LIST && seed_count && !seeds) return fail(c, "dxv_geodesic: a list of %u seeds at NULL", seed_count);
    if (seeds_kind == DXV_GEO_SEEDS_MASK && !seeds) return fail(c, "dxv_geodesic: the seed mask is NULL");
    if (check_whole_grid(c, "dxv_geodesic")) return 1;
    Frame& f = cur_frame(c);
    const uint32_t N = f.grid_dim;
    if (N > kGeoMaxN) return fail(c, "dxv_geodesic: a grid of %u^3 voxels; at most %u^3", N, kGeoMaxN);
    if (!geo_fits(N, metric))
        return fail(c, "dxv_geodesic: a grid of %u^3 voxels under metric %d: a path of weight %u per step can reach the codes of the map (wmax (N^3 - 1) must stay below 0xFFFFFFFE)", N,
                    metric, geo_max_weight(metric));
    const size_t voxels = (size_t)N * N * N;
    if (seeds_kind == DXV_GEO_SEEDS_LIST) {
        const uint32_t* list = static_cast<const uint32_t*>(seeds);
        for (uint32_t k = 0; k < seed_count; ++k)
            if (list[k] >= voxels) return fail(c, "dxv_geodesic: seed %u is voxel %u, outside the grid of %u^3 = %zu voxels", k, list[k], N, voxels);
    }
    DXV_HIP(c, hipSetDevice(c->device));
    if (seeds_kind == DXV_GEO_SEEDS_MASK) {
        size_t room = 0;
        const int r = check_device_range(c, "dxv_geodesic", seeds, voxels, &room);
        if (r == 2) return fail(c, "dxv_geodesic: the seed mask has %zu bytes from %p on, the grid has %zu voxels", room, seeds, voxels);
        if (r) return 1;
    }
    if (settle_frame_launch(c)) return 1;                               // (a pending fill, thin, expansion or geodesic of the frame first)
    const hipStream_t fs = cur_stream(c);
    const size_t scratch = geodesic_scratch_bytes(N);
    f.geoVersion = 0; f.geoDim = 0;
    DXV_HIP(c, f.geo.reserve(voxels, align256(voxels * sizeof(uint32_t)), fs));
    DXV_HIP(c, f.geoScratch.reserve(scratch, scratch, fs));
    const void* deviceSeeds = seeds;
    if (seeds_kind == DXV_GEO_SEEDS_LIST) {
        // the frame's own copy of the list (no geodesic of the frame is in flight: settle_frame_launch), uploaded from there
        const uint32_t* list = static_cast<const uint32_t*>(seeds);
        f.geoList.assign(list, list + seed_count);
        deviceSeeds = nullptr;
        if (seed_count) {
            DXV_HIP(c, f.geoSeeds.reserve(seed_count, align256((size_t)seed_count * sizeof(uint32_t)), fs));
            DXV_HIP(c, hipMemcpyAsync(f.geoSeeds.p, f.geoList.data(), (size_t)seed_count * sizeof(uint32_t), hipMemcpyHostToDevice, fs));
            deviceSeeds = f.geoSeeds.p;
        }
    }
    const bool timed = c->opt.events != 0;
    f.geoMetric = metric; f.geoLimit = limit;
    f.geoBatch = c->opt.georounds ? (uint32_t)c->opt.georounds : kGeoRoundsDefault;
    f.geoRounds = 0; f.geoTilesRun = 0; f.geoMostLive = 0; f.geoSparseRounds = 0;
    DXV_HIP(c, timer_begin(f.timers[kTimerGeodesic], timed, fs));
    DXV_HIP(c, launch_geodesic_init(f.grid.p, N, of, seeds_kind, deviceSeeds, seed_count, f.geo.p, f.geoScratch.p, fs));
    DXV_HIP(c, launch_geodesic_batch(f.geo.p, N, metric, limit, f.geoScratch.p, f.geoBatch, 0u, fs));
    DXV_HIP(c, timer_end(f.timers[kTimerGeodesic], timed, fs));
    DXV_HIP(c, hipMemcpyAsync(&c->pin->geoCtl[c->cur], f.geoScratch.p, sizeof(GeoControl), hipMemcpyDeviceToHost, fs));
    DXV_HIP(c, hipEventRecord(f.evEnd, fs));
    f.geoPending = true;
    f.geoDim = N; f.geoVersion = f.gridVersion;
    return 0;
}

int dxv_geodesic(dxv_ctx* c, int of, int metric, int seeds_kind, const void* seeds, uint32_t seed_count, uint32_t limit)
{
    if (dxv_geodesic_async(c, of, metric, seeds_kind, seeds, seed_count, limit)) return 1;
    return dxv_sync(c);
}

// whether the frame has a geodesic map to hand out: 0, or 1 with the reason as the message
static int current_geodesic(const dxv_ctx* c, const char* who)
{
    const Frame& f = c->frames[c->cur];
    dxv_ctx* w = const_cast<dxv_ctx*>(c);                               // (the message is the one thing an accessor writes)
    if (!f.geoDim || !f.geo.p) return fail(w, "%s: frame %u has no geodesic map yet (call dxv_geodesic first)", who, c->cur);
    if (f.geoVersion != f.gridVersion) return fail(w, "%s: frame %u was launched or edited again since its geodesic map was made: the map is stale", who, c->cur);
    return 0;
}

const void* dxv_geodesic_device_ptr(const dxv_ctx* c)
{
    if (!c || current_geodesic(c, "dxv_geodesic_device_ptr")) return nullptr;
    return c->frames[c->cur].geo.p;
}
size_t dxv_geodesic_bytes(const dxv_ctx* c)
{
    if (!c) return 0;
    const Frame& f = c->frames[c->cur];
    return f.geoDim && f.geoVersion == f.gridVersion ? (size_t)f.geoDim * f.geoDim * f.geoDim * sizeof(uint32_t) : 0;
}
int dxv_geodesic_download(dxv_ctx* c, void* host, size_t bytes)
{
    if (!c || current_geodesic(c, "dxv_geodesic_download")) return 1;
    return download_current(c, "dxv_geodesic_download", cur_frame(c).geo.p, dxv_geodesic_bytes(c), host, bytes);
}

int dxv_geodesic_info(dxv_ctx* c, float* ms, uint32_t* rounds, uint64_t* seeds_used, uint64_t* reached, uint64_t* unreached, uint32_t* farthest, uint32_t* farthest_voxel)
{
    if (!c || current_geodesic(c, "dxv_geodesic_info")) return 1;
    const Frame& f = cur_frame(c);
    if (ms) *ms = f.timers[kTimerGeodesic].ms;
    if (rounds) *rounds = f.geoRounds;
    if (seeds_used) *seeds_used = f.geoSeedsUsed;
    if (reached) *reached = f.geoReached;
    if (unreached) *unreached = f.geoUnreached;
    if (farthest) *farthest = f.geoFarthest;
    if (farthest_voxel) *farthest_voxel = f.geoFarthestVoxel;
    return 0;
}

int dxv_geodesic_work_info(dxv_ctx* c, uint64_t* tiles_run, uint32_t* most_live_tiles, uint32_t* sparse_rounds)
{
    if (!c || current_geodesic(c, "dxv_geodesic_work_info")) return 1;
    const Frame& f = cur_frame(c);
    if (tiles_run) *tiles_run = f.geoTilesRun;
    if (most_live_tiles) *most_live_tiles = f.geoMostLive;
    if (sparse_rounds) *sparse_rounds = f.geoSparseRounds;
    return 0;
}

// The path from `target` down to a seed of the selected frame's current map, synchronous: the frame is synchronised, the target's word is read,
// one wave walks down (geodesic.hip: k_geo_path) into the frame's own words, and min(length, capacity) of them come back.
int dxv_geodesic_path(dxv_ctx* c, uint32_t target, uint32_t* host_path, uint32_t capacity, uint32_t* length)
{
    if (!c || current_geodesic(c, "dxv_geodesic_path")) return 1;
    if (!length) return fail(c, "dxv_geodesic_path: length is NULL");
    if (capacity && !host_path) return fail(c, "dxv_geodesic_path: room for %u voxels at NULL", capacity);
    Frame& f = cur_frame(c);
    const uint32_t N = f.geoDim;
    const size_t voxels = (size_t)N * N * N;
    if (target >= voxels) return fail(c, "dxv_geodesic_path: target %u is outside the grid of %u^3 = %zu voxels", target, N, voxels);
    if (dxv_sync(c)) return 1;
    const hipStream_t fs = cur_stream(c);
    uint32_t word = 0;
    DXV_HIP(c, hipMemcpyAsync(&word, f.geo.p + target, sizeof(word), hipMemcpyDeviceToHost, fs));
    DXV_HIP(c, hipStreamSynchronize(fs));
    if (word >= kGeoUnreached)
        return fail(c, "dxv_geodesic_path: target %u holds no distance (%s)", target, word == kGeoNone ? "DXV_GEO_NONE: it is no member" : "DXV_GEO_UNREACHED: no path reaches it");
    const uint64_t longest = (uint64_t)word / geo_min_weight(f.geoMetric) + 1u;     // (every step lowers the word by the least weight or more)
    const uint32_t room = (uint64_t)capacity < longest ? capacity : (uint32_t)longest;
    DXV_HIP(c, f.geoPath.reserve((size_t)room + 2u, align256(((size_t)room + 2u) * sizeof(uint32_t)), fs));
    DXV_HIP(c, launch_geodesic_path(f.geo.p, N, f.geoMetric, target, f.geoPath.p, room, fs));
    uint32_t head[2] = {0, 0};
    DXV_HIP(c, hipMemcpyAsync(head, f.geoPath.p, sizeof(head), hipMemcpyDeviceToHost, fs));
    DXV_HIP(c, hipStreamSynchronize(fs));
    if (head[1] || head[0] > longest) return fail(c, "dxv_geodesic_path: no neighbour continues the path after %u voxels from target %u: the map is no fixed point", head[0], target);
    *length = head[0];
    const uint32_t give = head[0] < room ? head[0] : room;
    if (give) {
        DXV_HIP(c, hipMemcpyAsync(host_path, f.geoPath.p + 2, (size_t)give * sizeof(uint32_t), hipMemcpyDeviceToHost, fs));
        DXV_HIP(c, hipStreamSynchronize(fs));
    }
    return 0;
}

// The selected frame's grid edited from its labels (components.hip: k_comp_keep, k_comp_edit), in place, enqueued on the frame's stream behind
// whatever it holds -- under dxv_render_async's host-wait rule and dxv_fill_async's rules for the grid.  The four counters go into page-locked
// words and are read where the frame is next synchronised.
int dxv_components_select_async(dxv_ctx* c, int rule, uint32_t arg)
{
    if (!c) return 1;
    if (rule != DXV_SELECT_LARGEST && rule != DXV_SELECT_MIN_VOXELS && rule != DXV_SELECT_BORDER)
        return fail(c, "dxv_components_select: unknown rule %d (DXV_SELECT_LARGEST = 0, DXV_SELECT_MIN_VOXELS = 1, DXV_SELECT_BORDER = 2)", rule);
    if (rule != DXV_SELECT_MIN_VOXELS && arg) return fail(c, "dxv_components_select: rule %d takes no argument (arg must be 0, got %u)", rule, arg);
    if (current_labels(c, "dxv_components_select")) return 1;
    Frame& f = cur_frame(c);
    if (!f.grid.p || f.grid_dim != f.compDim || !frame_renderable(f))
        return fail(c, "dxv_components_select: the labels of frame %u do not belong to its grid: they are stale", c->cur);
    DXV_HIP(c, hipSetDevice(c->device));
    if (settle_frame_launch(c)) return 1;
    const hipStream_t fs = cur_stream(c);
    const uint32_t K = f.compCount;
    const size_t work = comp_select_bytes(K);
    DXV_HIP(c, f.compWork.reserve(work, work, fs));
    // the grid stops being what the frame's last launch wrote (dxv_fill_async's rules): a kept queue's zeros are gone, and whatever was made
    // of the grid before -- fields, the mesh, the tree, these labels -- is stale
    f.clearSig = 0;
    grid_rewritten(f);
    DXV_HIP(c, launch_comp_select(f.grid.p, f.compDim, f.compOf, f.compLabels.p, reinterpret_cast<const CompRecord*>(f.compTable.p), K, rule, arg, f.compWork.p, fs));
    DXV_HIP(c, hipMemcpyAsync(c->pin->compSel[c->cur], comp_select_counters(f.compWork.p), sizeof(c->pin->compSel[c->cur]), hipMemcpyDeviceToHost, fs));
    DXV_HIP(c, hipEventRecord(f.evEnd, fs));
    f.selPending = true; f.selRule = rule; f.selComponents = K;
    return 0;
}

int dxv_components_select(dxv_ctx* c, int rule, uint32_t arg)
{
    if (dxv_components_select_async(c, rule, arg)) return 1;
    return dxv_sync(c);
}

int dxv_components_select_info(dxv_ctx* c, uint32_t* kept, uint32_t* dropped, uint64_t* voxels_changed)
{
    if (!c) return 1;
    const Frame& f = cur_frame(c);
    if (kept) *kept = f.selKept;
    if (dropped) *dropped = f.selDropped;
    if (voxels_changed) *voxels_changed = f.selChanged;
    return 0;
}

// The exterior flood fill of the selected frame's grid (fill.hip), in place, enqueued on the frame's stream behind whatever it holds --
// under dxv_render_async's host-wait rule: one batch of rounds, the write-back, the batch's control block into page-locked words, the
// frame's end event.  Whether the batch converged is read where the frame is next synchronised (settle_fill).
int dxv_fill_async(dxv_ctx* c, int what)
{
    if (!c) return 1;
    if (what != DXV_FILL_SOLID && what != DXV_FILL_INTERIOR)
        return fail(c, "dxv_fill: unknown kind %d (DXV_FILL_SOLID = 0, DXV_FILL_INTERIOR = 1)", what);
    if (check_whole_grid(c, "dxv_fill")) return 1;
    Frame& f = cur_frame(c);
    DXV_HIP(c, hipSetDevice(c->device));
    if (settle_frame_launch(c)) return 1;
    const hipStream_t fs = cur_stream(c);
    const uint32_t N = f.grid_dim;
    const size_t scratch = fill_scratch_bytes(N);
    DXV_HIP(c, f.fillScratch.reserve(scratch, scratch, fs));
    const bool timed = c->opt.events != 0;
    f.fillWhat = what;
    f.fillBatch = c->opt.fillrounds ? (uint32_t)c->opt.fillrounds : kFillRoundsDefault;
    f.fillRounds = 0;
    // the grid stops being what the frame's last launch wrote: a kept queue's zeros are gone (the next launch clears everything; the
    // caller holds no pointer because of this, so ptrExposed stays), and a field made of the grid before is stale
    f.clearSig = 0;
    grid_rewritten(f);
    DXV_HIP(c, timer_begin(f.timers[kTimerFill], timed, fs));
    DXV_HIP(c, launch_fill(f.grid.p, N, what, f.fillScratch.p, f.fillBatch, true, fs));
    DXV_HIP(c, timer_end(f.timers[kTimerFill], timed, fs));
    DXV_HIP(c, hipMemcpyAsync(c->pin->fillCtl[c->cur], fill_control(f.fillScratch.p, N), sizeof(c->pin->fillCtl[c->cur]), hipMemcpyDeviceToHost, fs));
    DXV_HIP(c, hipEventRecord(f.evEnd, fs));
    f.fillPending = true;
    return 0;
}

int dxv_fill(dxv_ctx* c, int what)
{
    if (dxv_fill_async(c, what)) return 1;
    return dxv_sync(c);
}

int dxv_fill_info(dxv_ctx* c, float* ms, uint32_t* rounds)
{
    if (!c) return 1;
    if (ms) *ms = cur_frame(c).timers[kTimerFill].ms;
    if (rounds) *rounds = cur_frame(c).fillRounds;
    return 0;
}

// Morphology of the selected frame's grid by the Euclidean ball (morph.hip), in place, enqueued on the frame's stream behind whatever it holds
// -- under dxv_render_async's host-wait rule and dxv_fill_async's rules for the grid.  A fixed chain of kernels: nothing to settle; the two
// counters go into page-locked words and are read where the frame is next synchronised.
int dxv_morph_async(dxv_ctx* c, int op, uint32_t radius_sq)
{
    if (!c) return 1;
    if (op != DXV_MORPH_DILATE && op != DXV_MORPH_ERODE && op != DXV_MORPH_OPEN && op != DXV_MORPH_CLOSE)
        return fail(c, "dxv_morph: unknown operation %d (DXV_MORPH_DILATE = 0, DXV_MORPH_ERODE = 1, DXV_MORPH_OPEN = 2, DXV_MORPH_CLOSE = 3)", op);
    if (radius_sq < 1u || radius_sq > kMorphMaxRadiusSq)
        return fail(c, "dxv_morph: radius_sq %u is not in [1, %u]", radius_sq, kMorphMaxRadiusSq);
    if (check_whole_grid(c, "dxv_morph")) return 1;
    Frame& f = cur_frame(c);
    DXV_HIP(c, hipSetDevice(c->device));
    if (settle_frame_launch(c)) return 1;
    const hipStream_t fs = cur_stream(c);
    const uint32_t N = f.grid_dim;
    const int form = morph_form(radius_sq, c->opt.morphform);
    const size_t scratch = morph_scratch_bytes(N, op, radius_sq, form);
    DXV_HIP(c, f.morphScratch.reserve(scratch, scratch, fs));
    const bool timed = c->opt.events != 0;
    // the grid stops being what the frame's last launch wrote (dxv_fill_async's rules): a kept queue's zeros are gone, and whatever was made
    // of the grid before -- fields, the mesh, the tree, labels -- is stale
    f.clearSig = 0;
    grid_rewritten(f);
    DXV_HIP(c, timer_begin(f.timers[kTimerMorph], timed, fs));
    DXV_HIP(c, launch_morph(f.grid.p, N, op, radius_sq, form, f.morphScratch.p, fs));
    DXV_HIP(c, timer_end(f.timers[kTimerMorph], timed, fs));
    DXV_HIP(c, hipMemcpyAsync(c->pin->morphCount[c->cur], morph_counters(f.morphScratch.p), sizeof(c->pin->morphCount[c->cur]), hipMemcpyDeviceToHost, fs));
    DXV_HIP(c, hipEventRecord(f.evEnd, fs));
    f.morphPending = true;
    return 0;
}

int dxv_morph(dxv_ctx* c, int op, uint32_t radius_sq)
{
    if (dxv_morph_async(c, op, radius_sq)) return 1;
    return dxv_sync(c);
}

int dxv_morph_info(dxv_ctx* c, float* ms, uint64_t* voxels_set, uint64_t* voxels_cleared)
{
    if (!c) return 1;
    const Frame& f = cur_frame(c);
    if (ms) *ms = f.timers[kTimerMorph].ms;
    if (voxels_set) *voxels_set = f.morphSet;
    if (voxels_cleared) *voxels_cleared = f.morphCleared;
    return 0;
}

// Topology-preserving thinning of the selected frame's grid (thin.hip), in place, enqueued on the frame's stream behind whatever it holds -- under
// dxv_render_async's host-wait rule and dxv_fill_async's rules for the grid: one batch of iterations, the write-back, the batch's control block
// into page-locked words, the frame's end event.  Whether the batch reached the fixed point is read where the frame is next synchronised
// (settle_thin).
int dxv_thin_async(dxv_ctx* c, int kind, uint32_t max_iterations)
{
    if (!c) return 1;
    if (kind != DXV_THIN_CURVE && kind != DXV_THIN_KERNEL)
        return fail(c, "dxv_thin: unknown kind %d (DXV_THIN_CURVE = 0, DXV_THIN_KERNEL = 1)", kind);
    if (check_whole_grid(c, "dxv_thin")) return 1;
    Frame& f = cur_frame(c);
    DXV_HIP(c, hipSetDevice(c->device));
    if (settle_frame_launch(c)) return 1;
    const hipStream_t fs = cur_stream(c);
    const uint32_t N = f.grid_dim;
    if (N > kThinMaxN || (N & 1u)) return fail(c, "dxv_thin: a grid of side %u (needs an even side of at most %u)", N, kThinMaxN);
    const size_t scratch = thin_scratch_bytes(N);
    DXV_HIP(c, f.thinScratch.reserve(scratch, scratch, fs));
    const bool timed = c->opt.events != 0;
    f.thinKind = kind;
    f.thinBatch = c->opt.thinrounds ? (uint32_t)c->opt.thinrounds : kThinRoundsDefault;
    f.thinBounded = max_iterations != 0u;
    f.thinInBatch = thin_batch(f.thinBatch, max_iterations);
    f.thinLeft = f.thinBounded ? max_iterations - f.thinInBatch : 0u;
    f.thinIterations = 0;
    f.thinRemoved = 0;
    f.thinConverged = false;
    // the grid stops being what the frame's last launch wrote (dxv_fill_async's rules): a kept queue's zeros are gone, and whatever was made
    // of the grid before -- fields, the mesh, the tree, labels -- is stale
    f.clearSig = 0;
    grid_rewritten(f);
    DXV_HIP(c, timer_begin(f.timers[kTimerThin], timed, fs));
    DXV_HIP(c, launch_thin(f.grid.p, N, kind, f.thinScratch.p, f.thinInBatch, true, fs));
    DXV_HIP(c, timer_end(f.timers[kTimerThin], timed, fs));
    DXV_HIP(c, hipMemcpyAsync(&c->pin->thinCtl[c->cur], f.thinScratch.p, sizeof(ThinControl), hipMemcpyDeviceToHost, fs));
    DXV_HIP(c, hipEventRecord(f.evEnd, fs));
    f.thinPending = true;
    return 0;
}

int dxv_thin(dxv_ctx* c, int kind, uint32_t max_iterations)
{
    if (dxv_thin_async(c, kind, max_iterations)) return 1;
    return dxv_sync(c);
}

int dxv_thin_info(dxv_ctx* c, float* ms, uint32_t* iterations, uint64_t* voxels_removed, int* converged)
{
    if (!c) return 1;
    const Frame& f = cur_frame(c);
    if (ms) *ms = f.timers[kTimerThin].ms;
    if (iterations) *iterations = f.thinIterations;
    if (voxels_removed) *voxels_removed = f.thinRemoved;
    if (converged) *converged = f.thinConverged ? 1 : 0;
    return 0;
}
} // extern "C"
