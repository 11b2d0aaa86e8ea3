// dxv_products.hip -- what is made of a frame's grid, and what edits it in place: distance field, mesh distance field, isosurface, octree and
// its expansion, components, their measures and select, thickness, partition, skeleton graph and its prune, geodesic distance, access radius, fill, morph, thin -- the host side of each (the
// kernels: distance.hip, mesh_distance.hip, isosurface.hip, octree.hip, components.hip, measure.hip, thickness.hip, partition.hip, geodesic.hip,
// access.hip, skeleton.hip, fill.hip, morph.hip, thin.hip), the accessors of what they made, and their halves of a frame's synchronisation.  Each operator has a record in Frame (dxv_ctx.h);
// what they share is here, in front of them: the refusals (check_whole_grid, check_current), an operator's first and last steps (begin_operator,
// end_operator, blocking), a stage's own timer pair (StageTimer), the loop of the operators that run in batches (settle_batched), and what the two
// floods from seeds -- geodesic and access -- have alike: the seeds' refusals, their upload, the account of a batch, the work-info getter
// (check_seed_args, begin_seeded, upload_seeds, begin_flood, account_flood, flood_work_info).  What a caller READS of a product is a table: one
// descriptor per buffer (Readable) and three routines (product_ptr, product_bytes, product_download); every dxv_*_device_ptr, dxv_*_bytes and
// dxv_*_download entry is one line over them.  A new product's buffer is a descriptor and its three entries.
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
#include "dxv_partition.h"
#include "dxv_geodesic.h"
#include "dxv_access.h"
#include "dxv_sight.h"
#include "dxv_skeleton.h"

using namespace dxv;
using namespace dxvhost;

namespace dxvhost {

using PinnedFrame = dxv_ctx::Pinned::PerFrame;
static PinnedFrame& cur_pinned(dxv_ctx* c) { return c->pin->frame[c->cur]; }

// An operator's scratch laid out in the buffer it was reserved in: carve = the operator's own description (X_carve, args ..., params), the one
// its X_scratch_bytes sized the buffer with.  A buffer that does not hold what was taken fails the call here, in front of every launch.
template <class P, class F, class... A> static hipError_t carve_buffer(const DevBuf<uint8_t>& b, P& p, F carve, A... args)
{
    Carve c(b.p, b.cap);
    carve(c, args..., p);
    return b.p && c.fits() ? hipSuccess : hipErrorInvalidValue;
}

// the refusals of whatever works on the whole grid of the selected frame
static int check_whole_grid(dxv_ctx* c, const char* who)
{
    const Frame& f = cur_frame(c);
    if (!f.grid.p || !f.grid_dim) return fail(c, "%s: frame %u has no grid yet (call dxv_voxelize first)", who, c->cur);
    if (!frame_renderable(f)) return fail(c, "%s: needs the whole grid of the frame's last launch (z0 = 0, nz = grid_dim), not a slab or a share", who);
    return 0;
}

// What the refusals call a product: its noun, the call that makes it, and what is said once the grid has moved on.  The stale sentences
// differ from family to family on purpose -- each names what could have rewritten the grid when its product was added -- and dxv_isosurface
// speaks of a distance field in its own words.
struct ProductText { const char *noun, *maker, *stale; };
static const ProductText kDistanceText = {"distance field", "dxv_distance", "was launched again since its distance field was made: the field is stale"};
static const ProductText kDistanceTextOfIso = {"distance field", "dxv_distance", "was launched or filled again since its distance field was made: the field is stale"};
static const ProductText kMeshDistanceText = {"mesh distance field", "dxv_mesh_distance", "was launched or filled again since its mesh distance field was made: the field is stale"};
static const ProductText kIsoText = {"isosurface", "dxv_isosurface", "was launched or filled again since its isosurface was made: the mesh is stale"};
static const ProductText kOctreeText = {"octree", "dxv_octree", "was launched, filled or expanded again since its octree was made: the tree is stale"};
static const ProductText kComponentsText = {"components", "dxv_components",
                                            "was launched, filled, expanded or selected again since its components were labelled: labels and table are stale"};
static const ProductText kMeasureText = {"measure", "dxv_measure", "was launched, edited or labelled again since its components were measured: the measure is stale"};
static const ProductText kThicknessText = {"thickness map", "dxv_thickness", "was launched or edited again since its thickness map was made: map and histogram are stale"};
static const ProductText kPartitionText = {"partition", "dxv_partition", "was launched or edited again since its partition was made: labels, table and throats are stale"};
static const ProductText kGeodesicText = {"geodesic map", "dxv_geodesic", "was launched or edited again since its geodesic map was made: the map is stale"};
static const ProductText kSkeletonText = {"skeleton", "dxv_skeleton", "was launched or edited again since its skeleton was made: labels and tables are stale"};
static const ProductText kAccessText = {"access map", "dxv_access", "was launched or edited again since its access map was made: maps and histograms are stale"};
static const ProductText kSightText = {"line-of-sight map", "dxv_sight", "was launched or edited again since its line-of-sight map was made: map and tally are stale"};

// whether the selected frame has this product to hand out: 0, or 1 with the reason as the message
static int check_current(const dxv_ctx* c, const char* who, const Frame::Made& made, const ProductText& text)
{
    dxv_ctx* w = const_cast<dxv_ctx*>(c);                               // (the message is the one thing an accessor writes)
    if (!made.have) return fail(w, "%s: frame %u has no %s yet (call %s first)", who, c->cur, text.noun, text.maker);
    if (made.version != cur_frame(c).gridVersion) return fail(w, "%s: frame %u %s", who, c->cur, text.stale);
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

// What a caller reads of a product, one descriptor per buffer.  view: the record that guards the buffer, where the buffer is, its bytes as the
// record counts them, and whether the product was made with this part of it (the nearest triangles, the throats, the intrusion map are made on
// request) -- if not, `without` is the refusal, a format of (who, frame).  A buffer sized by a count is handed out as NULL, without a message,
// when the count is 0 (nullIfEmpty).  The measure alone is stale when another record, its labelling, is (ofLabels), and its size alone says why
// it is 0 (sizeSpeaks).
struct View { const Frame::Made* made; const void* p; size_t bytes; bool part = true; };
struct Readable {
    const ProductText& text;
    View (*view)(const Frame&);
    bool nullIfEmpty = false;
    const char* without = nullptr;
    bool ofLabels = false, sizeSpeaks = false;
};
static size_t cube(uint32_t n) { return (size_t)n * n * n; }
static const char kNoTriangles[] = "%s: frame %u's mesh distance field was made without triangles (want_triangles = 0)";
static const char kNoThroats[] = "%s: frame %u's partition was made without throats (want_throats = 0)";
static const char kNoIntrusion[] = "%s: the access map of frame %u was made without its intrusion map (call dxv_access with want_intrusion != 0)";

static const Readable kDistanceField = {kDistanceText, [](const Frame& f) { return View{&f.dist, f.dist.field.p, cube(f.dist.dim) * sizeof(int32_t)}; }};
static const Readable kMeshField = {kMeshDistanceText, [](const Frame& f) { return View{&f.mdist, f.mdist.field.p, (size_t)f.mdist.dim * f.mdist.dim * f.mdist.nz * sizeof(float)}; }};
static const Readable kMeshTriangles = {kMeshDistanceText, [](const Frame& f) { return View{&f.mdist, f.mdist.tri.p, (size_t)f.mdist.dim * f.mdist.dim * f.mdist.nz * sizeof(uint32_t), f.mdist.hasTri}; },
                                        false, kNoTriangles};
static const Readable kIsoVertices = {kIsoText, [](const Frame& f) { return View{&f.iso, f.iso.vb.p, (size_t)f.iso.vertices * sizeof(IsoVertex)}; }, true};
static const Readable kIsoIndices = {kIsoText, [](const Frame& f) { return View{&f.iso, f.iso.ib.p, (size_t)f.iso.triangles * 3u * sizeof(uint32_t)}; }, true};
static const Readable kOctreeNodes = {kOctreeText, [](const Frame& f) { return View{&f.oct, f.oct.nodes.p, (size_t)f.oct.count * 2u * sizeof(uint32_t)}; }};
static const Readable kCompLabels = {kComponentsText, [](const Frame& f) { return View{&f.comp, f.comp.labels.p, cube(f.comp.dim) * sizeof(uint32_t)}; }};
static const Readable kCompTable = {kComponentsText, [](const Frame& f) { return View{&f.comp, f.comp.table.p, (size_t)f.comp.count * sizeof(CompRecord)}; }, true};
static const Readable kMeasureTable = {kMeasureText, [](const Frame& f) { return View{&f.comp.measure, f.comp.measure.table.p, measure_table_bytes(f.comp.measure.count)}; },
                                       false, nullptr, true, true};
static const Readable kThickMap = {kThicknessText, [](const Frame& f) { return View{&f.thick, f.thick.map.p, cube(f.thick.dim) * sizeof(uint32_t)}; }};
static const Readable kThickHistogram = {kThicknessText, [](const Frame& f) { return View{&f.thick, f.thick.hist.p, thickness_histogram_bytes(f.thick.cap)}; }};
static const Readable kPartLabels = {kPartitionText, [](const Frame& f) { return View{&f.part, f.part.labels.p, cube(f.part.dim) * sizeof(uint32_t)}; }};
static const Readable kPartTable = {kPartitionText, [](const Frame& f) { return View{&f.part, f.part.table.p, (size_t)f.part.regions * sizeof(PartRegion)}; }, true};
static const Readable kPartThroats = {kPartitionText, [](const Frame& f) { return View{&f.part, f.part.throats.p, (size_t)f.part.throatCount * sizeof(PartThroat), f.part.hasThroats}; },
                                      true, kNoThroats};
static const Readable kSkelLabels = {kSkeletonText, [](const Frame& f) { return View{&f.skel, f.skel.labels.p, cube(f.skel.dim) * sizeof(uint32_t)}; }};
static const Readable kSkelNodes = {kSkeletonText, [](const Frame& f) { return View{&f.skel, f.skel.nodes.p, (size_t)f.skel.nodeCount * sizeof(SkelNode)}; }, true};
static const Readable kSkelBranches = {kSkeletonText, [](const Frame& f) { return View{&f.skel, f.skel.branches.p, (size_t)f.skel.branchCount * sizeof(SkelBranch)}; }, true};
static const Readable kGeoMap = {kGeodesicText, [](const Frame& f) { return View{&f.geo, f.geo.map.p, cube(f.geo.dim) * sizeof(uint32_t)}; }};
static const Readable kAccMap = {kAccessText, [](const Frame& f) { return View{&f.acc, f.acc.map.p, cube(f.acc.dim) * sizeof(uint32_t)}; }};
static const Readable kAccHistogram = {kAccessText, [](const Frame& f) { return View{&f.acc, f.acc.hist.p, thickness_histogram_bytes(f.acc.cap)}; }};
static const Readable kIntrusionMap = {kAccessText, [](const Frame& f) { return View{&f.acc, f.acc.intrusion.p, cube(f.acc.dim) * sizeof(uint32_t), f.acc.wantIntrusion}; },
                                       false, kNoIntrusion};
static const Readable kIntrusionHistogram = {kAccessText, [](const Frame& f) { return View{&f.acc, f.acc.histI.p, thickness_histogram_bytes(f.acc.cap), f.acc.wantIntrusion}; },
                                             false, kNoIntrusion};
static const Readable kSightMap = {kSightText, [](const Frame& f) { return View{&f.sight, f.sight.map.p, cube(f.sight.dim) * sizeof(uint32_t)}; }};

// whether the selected frame has this buffer to hand out, and *v, what it is: 0, or 1 -- with the reason as the message where an entry asks in
// its own name, without a word for who = nullptr
static int readable(const dxv_ctx* c, const char* who, const Readable& d, View* v)
{
    const Frame& f = cur_frame(c);
    *v = d.view(f);
    Frame::Made made = *v->made;
    if (d.ofLabels && f.comp.version != f.gridVersion) made.version = 0;    // (a measure of labels that are stale is stale)
    if (!who) return made.current(f) && v->part ? 0 : 1;
    if (check_current(c, who, made, d.text)) return 1;
    if (!v->part) return fail(const_cast<dxv_ctx*>(c), d.without, who, c->cur);
    return 0;
}
// dxv_*_device_ptr, dxv_*_bytes and dxv_*_download.  A download refuses in this order: the product, the part, the byte count (download_current).
static const void* product_ptr(const dxv_ctx* c, const char* who, const Readable& d)
{
    View v;
    if (!c || readable(c, who, d, &v)) return nullptr;
    return d.nullIfEmpty && !v.bytes ? nullptr : v.p;
}
static size_t product_bytes(const dxv_ctx* c, const char* who, const Readable& d)
{
    View v;
    return !c || readable(c, d.sizeSpeaks ? who : nullptr, d, &v) ? 0 : v.bytes;
}
static int product_download(dxv_ctx* c, const char* who, const Readable& d, void* host, size_t bytes)
{
    View v;
    if (!c || readable(c, who, d, &v)) return 1;
    return download_current(c, who, v.p, v.bytes, host, bytes);
}

// dxv_*_ms: the time the selected frame's last synchronisation read from one of its timers
static int timer_ms(dxv_ctx* c, const char* who, TimerUse use, float* ms)
{
    if (!c) return 1;
    if (!ms) return fail(c, "%s: ms is NULL", who);
    *ms = cur_frame(c).timers[use].ms;
    return 0;
}

// An operator's first step once it has refused what it must: the device, then dxv_render_async's host-wait rule -- the host waits for the
// selected frame only while it can still report something (settle_frame_launch) --, then the frame's stream, behind whatever it holds.
static int begin_operator(dxv_ctx* c, hipStream_t* fs)
{
    DXV_HIP(c, hipSetDevice(c->device));
    if (settle_frame_launch(c)) return 1;
    *fs = cur_stream(c);
    return 0;
}
// ... and its last: the second event of its timer (none: nullptr), what it reports into page-locked words for the frame's next
// synchronisation (none: nullptr), and the frame's end event, which nobody waits for here
static int end_operator(dxv_ctx* c, Frame& f, hipStream_t fs, Timer* t, void* words = nullptr, const void* counters = nullptr, size_t bytes = 0)
{
    if (t) DXV_HIP(c, timer_end(*t, c->opt.events != 0, fs));
    if (words) DXV_HIP(c, hipMemcpyAsync(words, counters, bytes, hipMemcpyDeviceToHost, fs));
    DXV_HIP(c, hipEventRecord(f.evEnd, fs));
    return 0;
}
// dxv_x(...) is dxv_x_async(...) and a synchronisation of the frame
static int blocking(dxv_ctx* c, int enqueued) { return enqueued ? 1 : dxv_sync(c); }

// A stage's own timer pair inside an operator that times the whole as well (options thickstages, partstages): recorded only for a caller that
// measures -- events on and the option set; for everybody else the stage reads 0 ms
struct StageTimer {
    Timer& t;
    bool staged;
    hipStream_t fs;
    hipError_t begin() const { if (!staged) t.ms = 0.0f; return timer_begin(t, staged, fs); }
    hipError_t end() const { return timer_end(t, staged, fs); }
};
static StageTimer stage_timer(const dxv_ctx* c, Frame& f, int slot, int option, hipStream_t fs) { return {f.timers[slot], c->opt.events != 0 && option != 0, fs}; }

// dxv_sync of one frame (sync_launch, once the stream has been waited for): the counters a select, a morph and a thickness left in page-locked words
void read_products(dxv_ctx* c, uint32_t i)
{
    Frame& f = c->frames[i];
    const PinnedFrame& pin = c->pin->frame[i];
    if (Frame::Components::Select& sel = f.comp.select; sel.pending) {  // the counters of the frame's last select (k_comp_keep has the LARGEST case)
        const bool largest = sel.rule == DXV_SELECT_LARGEST && sel.components;
        sel.kept = largest ? 1u : (uint32_t)pin.compSel[0];
        sel.dropped = largest ? sel.components - 1u : (uint32_t)pin.compSel[1];
        sel.changed = largest ? pin.compSel[2] - (pin.compSel[3] >> 32) : pin.compSel[2];
        sel.pending = false;
    }
    if (f.morph.pending) {                                              // the counters of the frame's last morph
        f.morph.set = pin.morphCount[0];
        f.morph.cleared = pin.morphCount[1];
        f.morph.pending = false;
    }
    if (f.thick.pending) {                                              // the counters of the frame's last thickness
        f.thick.centres = pin.thickCount[0];
        f.thick.items = pin.thickCount[1];
        f.thick.tested = pin.thickCount[2];
        f.thick.sent = pin.thickCount[3];
        f.thick.pending = false;
    }
    if (f.part.pending) {                                               // the counters of the frame's last partition
        f.part.cellsTested = pin.partCount[0];
        f.part.voxelsTested = pin.partCount[1];
        f.part.pending = false;
    }
    if (f.sight.pending) {                                              // the tally of the frame's last line-of-sight map
        memcpy(f.sight.tally, pin.sightTally, sizeof(f.sight.tally));
        f.sight.pending = false;
    }
    if (f.skel.prune.pending) {                                         // the counters of the frame's last prune
        f.skel.prune.branches = (uint32_t)pin.skelPrune[0];
        f.skel.prune.voxels = pin.skelPrune[1];
        f.skel.prune.pending = false;
    }
}

// ... and the half of an operator that runs in batches of rounds, behind it (the stream has been waited for): the verdict of the frame's last
// batch.  The batch's control block, in page-locked words by now, begins with a word per round: != 0, the round was live -- it still changed
// something.  A batch one of whose rounds was not live has reached the fixed point, that round confirming it.  Otherwise a further batch --
// from what the frame's scratch still holds -- is enqueued and waited for (the pattern of settle_lists: what only the host can decide is
// decided where the frame is synchronised anyway), its control block copied behind it, the timer's second event moved behind it.  Every
// live round reaches, removes or lowers at least one of the V voxels: the guard against an operator that never settles is V rounds.
struct Batched {
    const char *who, *unit;           // for the guard's message: "dxv_fill", "rounds"
    TimerUse timer;
    uint32_t N;                       // side of the grid the batches run on
    bool* pending;                    // a batch is in the stream whose verdict nobody has read yet
    uint32_t perBatch;                // rounds per batch ...
    const uint32_t* inStream;         // ... and of the batch in the stream (a bounded run's last batch is shorter)
    const uint32_t* done;             // rounds so far, for the guard's message
    void* ctl;                        // the control block in page-locked words ...
    const void* deviceCtl;            // ... and on the device, while a batch is pending
    size_t ctlBytes;
};
// account(live, last): the batch in the stream had `live` live rounds (last: and then one that was not) -- adds them to the frame's counters and
// says whether the operator is finished; launch(fs): sizes and enqueues the next batch.
template <class Account, class Launch> static int settle_batched(dxv_ctx* c, uint32_t i, const Batched& b, Account account, Launch launch)
{
    Frame& f = c->frames[i];
    const hipStream_t fs = frame_stream(c, i);
    const uint32_t* words = static_cast<const uint32_t*>(b.ctl);
    Timer& t = f.timers[b.timer];
    const uint64_t most = b.perBatch ? (uint64_t)b.N * b.N * b.N / b.perBatch + 2u : 0u;
    for (uint64_t batch = 0; *b.pending; ++batch) {
        uint32_t live = 0;
        while (live < *b.inStream && words[live]) ++live;
        if (account(live, live < *b.inStream)) {
            *b.pending = false;
            break;
        }
        if (batch >= most) return fail(c, "%s: no fixed point after %u %s on a grid of %u^3 voxels", b.who, *b.done, b.unit, b.N);
        DXV_HIP(c, launch(fs));
        if (t.armed) DXV_HIP(c, hipEventRecord(t.e1, fs));
        DXV_HIP(c, hipMemcpyAsync(b.ctl, b.deviceCtl, b.ctlBytes, hipMemcpyDeviceToHost, fs));
        DXV_HIP(c, hipEventRecord(f.evEnd, fs));
        DXV_HIP(c, hipStreamSynchronize(fs));
    }
    timer_read(t);
    return 0;
}

// the fill's: a batch whose last round still changed a word has not converged; a further batch is rounds and write-back from the masks
int settle_fill(dxv_ctx* c, uint32_t i)
{
    Frame& f = c->frames[i];
    Frame::Fill& o = f.fill;
    uint32_t* ctl = c->pin->frame[i].fillCtl;
    const uint32_t N = f.grid_dim;
    Carve carve(o.scratch.p, o.scratch.cap);                            // (as dxv_fill_async laid it out; all null without a scratch)
    FillScratch l{};
    fill_carve(carve, N, l);
    const Batched b{"dxv_fill", "rounds", kTimerFill, N, &o.pending, o.batch, &o.batch, &o.rounds, ctl, l.ctl, sizeof(c->pin->frame[i].fillCtl)};
    return settle_batched(c, i, b,
        [&](uint32_t live, bool last) { o.rounds += last ? live + 1u : o.batch; return last; },
        [&](hipStream_t fs) { return launch_fill(f.grid.p, N, o.what, l, o.batch, false, fs); });
}

// the thin's: a batch all of whose iterations removed something has not reached the fixed point; unless max_iterations has been used up, a
// further batch is iterations and write-back from the masks
int settle_thin(dxv_ctx* c, uint32_t i)
{
    Frame& f = c->frames[i];
    Frame::Thin& o = f.thin;
    ThinControl& ctl = c->pin->frame[i].thinCtl;
    const uint32_t N = f.grid_dim;
    Carve carve(o.scratch.p, o.scratch.cap);                            // (as dxv_thin_async laid it out; all null without a scratch)
    ThinScratch l{};
    thin_carve(carve, N, l);
    const Batched b{"dxv_thin", "iterations", kTimerThin, N, &o.pending, o.batch, &o.inBatch, &o.iterations, &ctl, l.ctl, sizeof(ThinControl)};
    return settle_batched(c, i, b,
        [&](uint32_t live, bool last) {
            o.removed = ctl.removed;
            o.iterations += last ? live + 1u : o.inBatch;
            if (last) o.converged = true;
            return last || (o.bounded && !o.left);                      // (... or max_iterations stopped it first)
        },
        [&](hipStream_t fs) {
            o.inBatch = thin_batch(o.batch, o.bounded ? o.left : 0u);
            if (o.bounded) o.left -= o.inBatch;
            return launch_thin(f.grid.p, N, o.kind, l, o.inBatch, false, fs);
        });
}

// The two floods from seeds, geodesic and access: word k of a batch's control block is the number of live tiles of round k, and the tally
// behind the rounds -- {seeds used, reached, unreached, the operator's own key} -- is read behind the confirming round only.  What the batch's
// live rounds ran (dxv_*_work_info), the rounds so far, and behind the last one the three counts of the tally that both keep:
static void account_flood(Frame::Flood& o, const GeoControl& ctl, uint32_t live, bool last)
{
    for (uint32_t k = 0; k < live; ++k) {
        o.tilesRun += ctl.live[k];
        if (ctl.live[k] > o.mostLive) o.mostLive = ctl.live[k];
        if (ctl.live[k] < kGeoSparseTiles) ++o.sparseRounds;
    }
    o.rounds += last ? live + 1u : o.batch;
    if (last) { o.seedsUsed = ctl.tally[0]; o.reached = ctl.tally[1]; o.unreached = ctl.tally[2]; }
}

// the geodesic's: a further batch is rounds from the flags the frame's scratch still holds, then the tally again
int settle_geodesic(dxv_ctx* c, uint32_t i)
{
    Frame& f = c->frames[i];
    Frame::Geodesic& o = f.geo;
    GeoControl& ctl = c->pin->frame[i].geoCtl;
    const uint32_t N = o.dim;
    Carve carve(o.scratch.p, o.scratch.cap);                            // (as dxv_geodesic_async laid it out; all null without a scratch)
    GeoScratch l{};
    geodesic_carve(carve, N, l);
    const Batched b{"dxv_geodesic", "rounds", kTimerGeodesic, N, &o.pending, o.batch, &o.batch, &o.rounds, &ctl, l.ctl, sizeof(GeoControl)};
    return settle_batched(c, i, b,
        [&](uint32_t live, bool last) {
            account_flood(o, ctl, live, last);
            if (last) {
                const GeoTally tally{ctl.tally[0], ctl.tally[1], ctl.tally[2], ctl.tally[3]};
                o.farthest = geo_tally_farthest(tally); o.farthestVoxel = geo_tally_farthest_voxel(tally);
            }
            return last;
        },
        [&](hipStream_t fs) { return launch_geodesic_batch(o.map.p, N, o.metric, o.limit, l, o.batch, o.rounds, fs); });
}

// the access's: the geodesic's loop; behind the confirming round A is final, and what is made of it -- A into the radius field, thickness's
// stages TOP .. HISTOGRAM with W = the intrusion map, A's own histogram -- is enqueued here and waited for, the timer's second event behind it
static AccScratch access_scratch(const Frame::Access& o)
{
    Carve carve(o.scratch.p, o.scratch.cap);                            // (as dxv_access_async laid it out; all null without a scratch)
    AccScratch l{};
    access_carve(carve, o.dim, o.wantIntrusion, l);
    return l;
}
static ThickParams access_params(const Frame::Access& o, uint32_t* W, unsigned long long* hist)
{
    ThickParams p = access_scratch(o).thick;
    p.of = o.of; p.cap = o.cap; p.cull = o.cull; p.count = 0u; p.W = W; p.hist = hist;
    return p;
}
static int finish_access(dxv_ctx* c, uint32_t i)
{
    Frame& f = c->frames[i];
    Frame::Access& o = f.acc;
    const hipStream_t fs = frame_stream(c, i);
    Timer& t = f.timers[kTimerAccess];
    DXV_HIP(c, launch_thickness_stage(f.grid.p, access_params(o, o.map.p, o.hist.p), THICK_STAGE_HISTOGRAM, fs));
    if (o.wantIntrusion) {
        const ThickParams p = access_params(o, o.intrusion.p, o.histI.p);
        DXV_HIP(c, launch_access_radius(o.map.p, o.dim, o.of, access_scratch(o), fs));
        for (int stage = THICK_STAGE_TOP; stage < THICK_STAGES; ++stage) DXV_HIP(c, launch_thickness_stage(f.grid.p, p, stage, fs));
    }
    if (t.armed) DXV_HIP(c, hipEventRecord(t.e1, fs));
    DXV_HIP(c, hipEventRecord(f.evEnd, fs));
    DXV_HIP(c, hipStreamSynchronize(fs));
    return 0;
}
int settle_access(dxv_ctx* c, uint32_t i)
{
    Frame& f = c->frames[i];
    Frame::Access& o = f.acc;
    GeoControl& ctl = c->pin->frame[i].accCtl;
    const uint32_t N = o.dim;
    int finished = 0;
    const AccScratch l = access_scratch(o);
    const Batched b{"dxv_access", "rounds", kTimerAccess, N, &o.pending, o.batch, &o.batch, &o.rounds, &ctl, l.ctl, sizeof(GeoControl)};
    const int r = settle_batched(c, i, b,
        [&](uint32_t live, bool last) {
            account_flood(o, ctl, live, last);
            if (last) {
                const AccTally tally{ctl.tally[0], ctl.tally[1], ctl.tally[2], ctl.tally[3]};
                o.widest = acc_tally_widest(tally); o.widestVoxel = acc_tally_widest_voxel(tally);
                finished = finish_access(c, i);
            }
            return last;
        },
        [&](hipStream_t fs) { return launch_access_batch(o.map.p, N, o.of, o.connectivity, o.cap, l, o.batch, o.rounds, fs); });
    return r ? r : finished;
}

// ... and the verdict of an expansion from a caller's tree (sync_launch has read the word): an index that could not be followed left empty
// voxels behind and is reported here, once
int settle_expand(dxv_ctx* c, uint32_t i)
{
    Frame& f = c->frames[i];
    if (!f.oct.expandPending) return 0;
    f.oct.expandPending = false;
    if (!c->pin->frame[i].status[kOctStatusWord]) return 0;
    DXV_HIP(c, hipMemsetAsync(f.status.p + kOctStatusWord, 0, sizeof(uint32_t), frame_stream(c, i)));
    return fail(c, "dxv_octree_expand: the tree given for frame %u cannot be followed (a child index at or beyond its node count, or cells still mixed "
                   "after all its levels); the voxels behind such an index were left empty", i);
}

// The seeds of a flood, as dxv_geodesic_async and dxv_access_async take them.  What is refused of them in front of check_whole_grid ...
static int check_seed_args(dxv_ctx* c, const char* who, int kind, const void* seeds, uint32_t count)
{
    if (kind != DXV_GEO_SEEDS_BORDER && kind != DXV_GEO_SEEDS_LIST && kind != DXV_GEO_SEEDS_MASK)
        return fail(c, "%s: unknown seed kind %d (DXV_GEO_SEEDS_BORDER = 0, DXV_GEO_SEEDS_LIST = 1, DXV_GEO_SEEDS_MASK = 2)", who, kind);
    if (kind == DXV_GEO_SEEDS_LIST && count && !seeds) return fail(c, "%s: a list of %u seeds at NULL", who, count);
    if (kind == DXV_GEO_SEEDS_MASK && !seeds) return fail(c, "%s: the seed mask is NULL", who);
    return 0;
}
// ... and behind the refusals of the grid's size, as the operator's first step: begin_operator's steps with the device in front of the range
// check of a mask -- a list's values against the grid, the device, a mask's range, then the host-wait rule (a pending fill, thin, expansion or
// flood of the frame first) and the frame's stream
static int begin_seeded(dxv_ctx* c, const char* who, int kind, const void* seeds, uint32_t count, uint32_t N, hipStream_t* fs)
{
    const size_t voxels = cube(N);
    if (kind == DXV_GEO_SEEDS_LIST) {
        const uint32_t* list = static_cast<const uint32_t*>(seeds);
        for (uint32_t k = 0; k < count; ++k)
            if (list[k] >= voxels) return fail(c, "%s: seed %u is voxel %u, outside the grid of %u^3 = %zu voxels", who, k, list[k], N, voxels);
    }
    DXV_HIP(c, hipSetDevice(c->device));
    if (kind == DXV_GEO_SEEDS_MASK) {
        size_t room = 0;
        const int r = check_device_range(c, who, seeds, voxels, &room);
        if (r == 2) return fail(c, "%s: the seed mask has %zu bytes from %p on, the grid has %zu voxels", who, room, seeds, voxels);
        if (r) return 1;
    }
    if (settle_frame_launch(c)) return 1;
    *fs = cur_stream(c);
    return 0;
}
// ... and what the init kernel is given: a mask as it is; a list as the frame's own copy (no flood of the frame is in flight:
// settle_frame_launch), uploaded from there -- nullptr for an empty one
static int upload_seeds(dxv_ctx* c, Frame::Flood& o, int kind, const void* seeds, uint32_t count, hipStream_t fs, const void** deviceSeeds)
{
    *deviceSeeds = seeds;
    if (kind != DXV_GEO_SEEDS_LIST) return 0;
    const uint32_t* list = static_cast<const uint32_t*>(seeds);
    o.list.assign(list, list + count);
    *deviceSeeds = nullptr;
    if (count) {
        DXV_HIP(c, o.seeds.reserve(count, align256((size_t)count * sizeof(uint32_t)), fs));
        DXV_HIP(c, hipMemcpyAsync(o.seeds.p, o.list.data(), (size_t)count * sizeof(uint32_t), hipMemcpyHostToDevice, fs));
        *deviceSeeds = o.seeds.p;
    }
    return 0;
}
// a flood starts: rounds per batch from its option (0: the operator's default), nothing run yet
static void begin_flood(Frame::Flood& o, int option, uint32_t roundsDefault)
{
    o.batch = option ? (uint32_t)option : roundsDefault;
    o.rounds = 0; o.tilesRun = 0; o.mostLive = 0; o.sparseRounds = 0;
}
// dxv_geodesic_work_info, dxv_access_work_info
static int flood_work_info(dxv_ctx* c, const char* who, const Frame::Flood& o, const ProductText& text, uint64_t* tiles_run, uint32_t* most_live_tiles, uint32_t* sparse_rounds)
{
    if (check_current(c, who, o, text)) return 1;
    if (tiles_run) *tiles_run = o.tilesRun;
    if (most_live_tiles) *most_live_tiles = o.mostLive;
    if (sparse_rounds) *sparse_rounds = o.sparseRounds;
    return 0;
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
    hipStream_t fs;
    if (begin_operator(c, &fs)) return 1;
    const uint32_t N = f.grid_dim;
    const size_t voxels = (size_t)N * N * N, scratch = distance_scratch_bytes(N);
    f.dist.version = 0; f.dist.have = false;
    DXV_HIP(c, f.dist.field.reserve(voxels, align256(voxels * sizeof(int32_t)), fs));
    DXV_HIP(c, f.dist.scratch.reserve(scratch, scratch, fs));
    DXV_HIP(c, timer_begin(f.timers[kTimerDistance], c->opt.events != 0, fs));
    DXV_HIP(c, launch_distance(f.grid.p, N, format, f.dist.field.p, f.dist.scratch.p, fs));
    if (end_operator(c, f, fs, &f.timers[kTimerDistance])) return 1;
    f.dist.dim = N; f.dist.format = format; f.dist.have = true; f.dist.version = f.gridVersion;
    return 0;
}

int dxv_distance(dxv_ctx* c, int format) { return blocking(c, dxv_distance_async(c, format)); }

const void* dxv_distance_device_ptr(const dxv_ctx* c) { return product_ptr(c, "dxv_distance_device_ptr", kDistanceField); }
size_t dxv_distance_bytes(const dxv_ctx* c) { return product_bytes(c, "dxv_distance_bytes", kDistanceField); }
int dxv_distance_download(dxv_ctx* c, void* host, size_t bytes) { return product_download(c, "dxv_distance_download", kDistanceField, host, bytes); }

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
    hipStream_t fs;
    if (begin_operator(c, &fs)) return 1;
    const bool walk = c->opt.mdistwalk != 0;
    if (walk && ensure_nodes(c, fs)) return 1;                          // after a refit that deferred the node boxes, as before a tree walk
    const uint32_t N = f.grid_dim;
    const size_t voxels = (size_t)N * N * f.nz;
    f.mdist.version = 0; f.mdist.have = false;
    DXV_HIP(c, f.mdist.field.reserve(voxels, align256(voxels * sizeof(float)), fs));
    if (wantTriangles) DXV_HIP(c, f.mdist.tri.reserve(voxels, align256(voxels * sizeof(uint32_t)), fs));
    MeshDistanceParams p{};
    p.grid = f.grid.p; p.field = f.mdist.field.p; p.tris = wantTriangles ? f.mdist.tri.p : nullptr;
    p.N = N; p.z0 = f.z0; p.nz = f.nz;
    p.format = format;
    p.cap = md_cap(N, bandVoxels);
    p.cullAbs = md_cull_abs(c->hdr.rootLo, c->hdr.rootHi);
    DXV_HIP(c, timer_begin(f.timers[kTimerMeshDistance], c->opt.events != 0, fs));
    DXV_HIP(c, launch_mesh_distance(scene_nodes(c), scene_tripos(c), c->hdr.numTris, p, walk, fs));
    if (end_operator(c, f, fs, &f.timers[kTimerMeshDistance])) return 1;
    f.sceneReadPending = true;
    f.mdist.dim = N; f.mdist.nz = f.nz; f.mdist.format = format; f.mdist.hasTri = wantTriangles != 0; f.mdist.have = true; f.mdist.version = f.gridVersion;
    return 0;
}

int dxv_mesh_distance(dxv_ctx* c, int format, uint32_t bandVoxels, int wantTriangles) { return blocking(c, dxv_mesh_distance_async(c, format, bandVoxels, wantTriangles)); }

// (the nearest triangles have the field's size: there is no size of their own)
const void* dxv_mesh_distance_device_ptr(const dxv_ctx* c) { return product_ptr(c, "dxv_mesh_distance_device_ptr", kMeshField); }
const void* dxv_mesh_distance_triangles_device_ptr(const dxv_ctx* c) { return product_ptr(c, "dxv_mesh_distance_triangles_device_ptr", kMeshTriangles); }
size_t dxv_mesh_distance_bytes(const dxv_ctx* c) { return product_bytes(c, "dxv_mesh_distance_bytes", kMeshField); }
int dxv_mesh_distance_download(dxv_ctx* c, void* host, size_t bytes) { return product_download(c, "dxv_mesh_distance_download", kMeshField, host, bytes); }
int dxv_mesh_distance_triangles_download(dxv_ctx* c, void* host, size_t bytes) { return product_download(c, "dxv_mesh_distance_triangles_download", kMeshTriangles, host, bytes); }

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
        if (check_current(c, "dxv_isosurface", f.mdist, kMeshDistanceText)) return 1;
        if (f.mdist.nz != f.mdist.dim)
            return fail(c, "dxv_isosurface: the frame's mesh distance field is a slab's (%u of %u slices); needs the field of the whole grid", f.mdist.nz, f.mdist.dim);
        field = f.mdist.field.p; N = f.mdist.dim;
        if (f.mdist.format == DXV_MDIST_UNITS_F32) P = 2.0f / (float)N;
    } else {
        if (check_current(c, "dxv_isosurface", f.dist, kDistanceTextOfIso)) return 1;
        if (f.dist.format != DXV_DIST_F32) return fail(c, "dxv_isosurface: the frame's distance field is in the int32 format; needs DXV_DIST_F32");
        field = reinterpret_cast<const float*>(f.dist.field.p); N = f.dist.dim;
    }
    if (space == DXV_ISO_SPACE_OBJECT && !c->haveScene)
        return fail(c, "dxv_isosurface: DXV_ISO_SPACE_OBJECT needs the scene's bound and the context has no scene (call dxv_build or dxv_scene_import, or ask for DXV_ISO_SPACE_VOXELS)");
    hipStream_t fs;
    if (begin_operator(c, &fs)) return 1;
    const size_t scratch = iso_scratch_bytes(N);
    DXV_HIP(c, f.iso.scratch.reserve(scratch, scratch, fs));
    IsoParams p{};
    p.field = field; p.N = N; p.iso = iso; p.P = P; p.object = space == DXV_ISO_SPACE_OBJECT;
    memcpy(p.bound, c->bound, sizeof(p.bound));
    DXV_HIP(c, carve_buffer(f.iso.scratch, p, iso_carve, N));
    unsigned long long* totals = cur_pinned(c).isoTotals;
    DXV_HIP(c, timer_begin(f.timers[kTimerIso], c->opt.events != 0, fs));
    DXV_HIP(c, launch_iso_count(p, fs));
    DXV_HIP(c, hipMemcpyAsync(totals, p.totals, 2 * sizeof(unsigned long long), hipMemcpyDeviceToHost, fs));
    DXV_HIP(c, hipStreamSynchronize(fs));
    const unsigned long long vertices = totals[0], quads = totals[1];
    if (vertices > kIsoMaxCount || quads > kIsoMaxCount / 6u)
        return fail(c, "dxv_isosurface: a mesh of %llu vertices and %llu index words; at most %llu of each (the frame's earlier mesh is kept)", vertices,
                    6u * quads, (unsigned long long)kIsoMaxCount);
    f.iso.version = 0;
    if (vertices) {
        DXV_HIP(c, f.iso.vb.reserve((size_t)vertices, align256((size_t)vertices * sizeof(IsoVertex)), fs));
        if (quads) DXV_HIP(c, f.iso.ib.reserve(6 * (size_t)quads, align256(6 * (size_t)quads * sizeof(uint32_t)), fs));
        p.vb = reinterpret_cast<IsoVertex*>(f.iso.vb.p); p.ib = f.iso.ib.p;
        DXV_HIP(c, launch_iso_emit(p, fs));
    }
    if (end_operator(c, f, fs, &f.timers[kTimerIso])) return 1;
    f.iso.vertices = (uint32_t)vertices; f.iso.triangles = (uint32_t)(2u * quads);
    f.iso.have = true; f.iso.version = f.gridVersion;
    return 0;
}

int dxv_isosurface(dxv_ctx* c, int source, float iso, int space) { return blocking(c, dxv_isosurface_async(c, source, iso, space)); }

int dxv_isosurface_counts(dxv_ctx* c, uint32_t* vertices, uint32_t* triangles)
{
    if (!c || check_current(c, "dxv_isosurface_counts", cur_frame(c).iso, kIsoText)) return 1;
    if (vertices) *vertices = cur_frame(c).iso.vertices;
    if (triangles) *triangles = cur_frame(c).iso.triangles;
    return 0;
}

// (dxv_isosurface_counts gives the sizes: the mesh has no dxv_*_bytes)
const void* dxv_isosurface_vertices_device_ptr(const dxv_ctx* c) { return product_ptr(c, "dxv_isosurface_vertices_device_ptr", kIsoVertices); }
const void* dxv_isosurface_indices_device_ptr(const dxv_ctx* c) { return product_ptr(c, "dxv_isosurface_indices_device_ptr", kIsoIndices); }
int dxv_isosurface_vertices_download(dxv_ctx* c, void* host, size_t bytes) { return product_download(c, "dxv_isosurface_vertices_download", kIsoVertices, host, bytes); }
int dxv_isosurface_indices_download(dxv_ctx* c, void* host, size_t bytes) { return product_download(c, "dxv_isosurface_indices_download", kIsoIndices, host, bytes); }

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
    hipStream_t fs;
    if (begin_operator(c, &fs)) return 1;
    const uint32_t N = f.grid_dim;
    const size_t scratch = oct_scratch_bytes(N);
    DXV_HIP(c, f.oct.scratch.reserve(scratch, scratch, fs));
    OctParams p{};
    p.grid = f.grid.p;
    DXV_HIP(c, carve_buffer(f.oct.scratch, p, oct_carve, N));
    const uint32_t L = p.L;
    unsigned long long* totals = cur_pinned(c).octTotals;
    DXV_HIP(c, timer_begin(f.timers[kTimerOctree], c->opt.events != 0, fs));
    DXV_HIP(c, launch_oct_count(p, fs));
    DXV_HIP(c, hipMemcpyAsync(totals, p.levelFirst, (L + 1u) * sizeof(unsigned long long), hipMemcpyDeviceToHost, fs));
    DXV_HIP(c, hipStreamSynchronize(fs));
    const unsigned long long nodes = totals[L];
    if (!nodes || nodes > kOctMaxNodes)
        return fail(c, "dxv_octree: a tree of %llu nodes; at least the root and at most %llu (the frame's earlier tree is kept)", nodes,
                    (unsigned long long)kOctMaxNodes);
    f.oct.version = 0;
    DXV_HIP(c, f.oct.nodes.reserve((size_t)nodes, align256((size_t)nodes * 2u * sizeof(uint32_t)), fs));
    p.nodes = f.oct.nodes.p;
    DXV_HIP(c, launch_oct_emit(p, fs));
    if (end_operator(c, f, fs, &f.timers[kTimerOctree])) return 1;
    f.oct.levels = L; f.oct.count = (uint32_t)nodes;
    for (uint32_t l = 0; l < 12u; ++l) f.oct.levelFirst[l] = l <= L ? (uint32_t)totals[l] : 0u;
    f.oct.have = true; f.oct.version = f.gridVersion;
    return 0;
}

int dxv_octree(dxv_ctx* c) { return blocking(c, dxv_octree_async(c)); }

int dxv_octree_info(dxv_ctx* c, uint32_t* levels, uint32_t* nodes, uint32_t level_first[12])
{
    if (!c || check_current(c, "dxv_octree_info", cur_frame(c).oct, kOctreeText)) return 1;
    const Frame& f = cur_frame(c);
    if (levels) *levels = f.oct.levels;
    if (nodes) *nodes = f.oct.count;
    if (level_first) memcpy(level_first, f.oct.levelFirst, sizeof(f.oct.levelFirst));
    return 0;
}

const void* dxv_octree_device_ptr(const dxv_ctx* c) { return product_ptr(c, "dxv_octree_device_ptr", kOctreeNodes); }
size_t dxv_octree_bytes(const dxv_ctx* c) { return product_bytes(c, "dxv_octree_bytes", kOctreeNodes); }
int dxv_octree_download(dxv_ctx* c, void* host, size_t bytes) { return product_download(c, "dxv_octree_download", kOctreeNodes, host, bytes); }

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
        if (check_current(c, "dxv_octree_expand", f.oct, kOctreeText)) return 1;
        deviceNodes = f.oct.nodes.p; nodes = f.oct.count;               // (a current tree is the tree of this grid: its levels are L)
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
    if (settle_frame_launch(c)) return 1;                               // (begin_operator's steps, the device in front of the range check)
    const hipStream_t fs = cur_stream(c);
    edited_in_place(f);                                                 // (the frame's own tree is stale with the rest)
    DXV_HIP(c, launch_oct_expand(f.grid.p, N, static_cast<const uint32_t*>(deviceNodes), nodes, f.status.p + kOctStatusWord, fs));
    if (end_operator(c, f, fs, nullptr)) return 1;
    if (!own) f.oct.expandPending = true;                               // (the frame's own tree was made by the build: it has nothing to report)
    return 0;
}

int dxv_octree_expand(dxv_ctx* c, const void* deviceNodes, uint32_t nodes, uint32_t levels) { return blocking(c, dxv_octree_expand_async(c, deviceNodes, nodes, levels)); }

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
    hipStream_t fs;
    if (begin_operator(c, &fs)) return 1;
    const size_t voxels = (size_t)N * N * N, scratch = comp_scratch_bytes(N);
    DXV_HIP(c, f.comp.scratch.reserve(scratch, scratch, fs));
    f.comp.version = 0;                                                 // (the build writes into the frame's label buffer: what it held is gone)
    f.comp.measure.version = 0;                                         // (... and a measure of the labels it held with it)
    DXV_HIP(c, f.comp.labels.reserve(voxels, align256(voxels * sizeof(uint32_t)), fs));
    CompParams p{};
    p.grid = f.grid.p; p.of = of; p.connectivity = (uint32_t)connectivity; p.labels = f.comp.labels.p;
    DXV_HIP(c, carve_buffer(f.comp.scratch, p, comp_carve, N));
    unsigned long long* total = &cur_pinned(c).compTotal;
    DXV_HIP(c, timer_begin(f.timers[kTimerComponents], c->opt.events != 0, fs));
    DXV_HIP(c, launch_comp_label(p, fs));
    DXV_HIP(c, hipMemcpyAsync(total, p.total, sizeof(unsigned long long), hipMemcpyDeviceToHost, fs));
    DXV_HIP(c, hipStreamSynchronize(fs));
    const uint32_t K = (uint32_t)*total;
    if (K) {
        DXV_HIP(c, f.comp.table.reserve(K, align256((size_t)K * sizeof(CompRecord)), fs));
        DXV_HIP(c, f.comp.work.reserve((size_t)K * sizeof(CompStats), align256((size_t)K * sizeof(CompStats)), fs));
        p.table = reinterpret_cast<CompRecord*>(f.comp.table.p);
        p.stats = reinterpret_cast<CompStats*>(f.comp.work.p);
        DXV_HIP(c, launch_comp_stats(p, K, fs));
    }
    if (end_operator(c, f, fs, &f.timers[kTimerComponents])) return 1;
    f.comp.count = K; f.comp.dim = N; f.comp.of = of; f.comp.connectivity = connectivity;
    f.comp.have = true; f.comp.version = f.gridVersion;
    return 0;
}

int dxv_components(dxv_ctx* c, int of, int connectivity) { return blocking(c, dxv_components_async(c, of, connectivity)); }

int dxv_components_info(dxv_ctx* c, uint32_t* count, int* of, int* connectivity)
{
    if (!c || check_current(c, "dxv_components_info", cur_frame(c).comp, kComponentsText)) return 1;
    const Frame& f = cur_frame(c);
    if (count) *count = f.comp.count;
    if (of) *of = f.comp.of;
    if (connectivity) *connectivity = f.comp.connectivity;
    return 0;
}

const void* dxv_components_labels_device_ptr(const dxv_ctx* c) { return product_ptr(c, "dxv_components_labels_device_ptr", kCompLabels); }
size_t dxv_components_labels_bytes(const dxv_ctx* c) { return product_bytes(c, "dxv_components_labels_bytes", kCompLabels); }
int dxv_components_labels_download(dxv_ctx* c, void* host, size_t bytes) { return product_download(c, "dxv_components_labels_download", kCompLabels, host, bytes); }
const void* dxv_components_table_device_ptr(const dxv_ctx* c) { return product_ptr(c, "dxv_components_table_device_ptr", kCompTable); }
size_t dxv_components_table_bytes(const dxv_ctx* c) { return product_bytes(c, "dxv_components_table_bytes", kCompTable); }
int dxv_components_table_download(dxv_ctx* c, void* host, size_t bytes) { return product_download(c, "dxv_components_table_download", kCompTable, host, bytes); }

int dxv_components_ms(dxv_ctx* c, float* ms) { return timer_ms(c, "dxv_components_ms", kTimerComponents, ms); }

// The integral measures of the selected frame's current labelling (measure.hip; dxv_measure.h has the rule's routines), enqueued on the frame's
// stream behind whatever it holds, under dxv_render_async's host-wait rule.  K is known from the labelling: nothing is read back.  The member
// mask is the labelling's own; once dxv_trim has released it, it is packed again from the grid, which a current labelling guarantees unchanged.
int dxv_measure_async(dxv_ctx* c)
{
    if (!c) return 1;
    if (check_whole_grid(c, "dxv_measure")) return 1;
    if (check_current(c, "dxv_measure", cur_frame(c).comp, kComponentsText)) return 1;
    Frame& f = cur_frame(c);
    if (f.grid_dim != f.comp.dim) return fail(c, "dxv_measure: the labels of frame %u do not belong to its grid: they are stale", c->cur);
    hipStream_t fs;
    if (begin_operator(c, &fs)) return 1;
    const uint32_t N = f.comp.dim, K = f.comp.count;
    const bool packed = f.comp.scratch.p != nullptr;                    // (the mask of the frame's last labelling: this one, it is current)
    const size_t scratch = comp_scratch_bytes(N);
    DXV_HIP(c, f.comp.scratch.reserve(scratch, scratch, fs));
    f.comp.measure.version = 0;
    DXV_HIP(c, f.comp.measure.table.reserve((size_t)K + 1u, align256(measure_table_bytes(K)), fs));
    CompParams p{};
    DXV_HIP(c, carve_buffer(f.comp.scratch, p, comp_carve, N));
    DXV_HIP(c, timer_begin(f.timers[kTimerMeasure], c->opt.events != 0, fs));
    if (!packed) DXV_HIP(c, launch_comp_pack(f.grid.p, N, f.comp.of, p.mask, fs));
    DXV_HIP(c, launch_measure(p.mask, N, (uint32_t)f.comp.connectivity, f.comp.labels.p, K, f.comp.measure.table.p, fs));
    if (end_operator(c, f, fs, &f.timers[kTimerMeasure])) return 1;
    f.comp.measure.count = K; f.comp.measure.have = true; f.comp.measure.version = f.gridVersion;
    return 0;
}

int dxv_measure(dxv_ctx* c) { return blocking(c, dxv_measure_async(c)); }

// (the one size that says why it is 0: kMeasureTable)
const void* dxv_measure_table_device_ptr(const dxv_ctx* c) { return product_ptr(c, "dxv_measure_table_device_ptr", kMeasureTable); }
size_t dxv_measure_table_bytes(const dxv_ctx* c) { return product_bytes(c, "dxv_measure_table_bytes", kMeasureTable); }
int dxv_measure_table_download(dxv_ctx* c, void* host, size_t bytes) { return product_download(c, "dxv_measure_table_download", kMeasureTable, host, bytes); }

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
    hipStream_t fs;
    if (begin_operator(c, &fs)) return 1;
    const size_t voxels = (size_t)N * N * N, scratch = thickness_scratch_bytes(N);
    f.thick.version = 0; f.thick.have = false;
    DXV_HIP(c, f.thick.map.reserve(voxels, align256(voxels * sizeof(uint32_t)), fs));
    DXV_HIP(c, f.thick.hist.reserve(kThickMaxCapSq + 1u, align256(thickness_histogram_bytes(kThickMaxCapSq)), fs));
    DXV_HIP(c, f.thick.scratch.reserve(scratch, scratch, fs));
    ThickParams p{};
    p.of = of; p.cap = cap_sq; p.cull = (uint32_t)c->opt.thickcull; p.count = c->opt.thickstages ? 1u : 0u; p.W = f.thick.map.p; p.hist = f.thick.hist.p;
    DXV_HIP(c, carve_buffer(f.thick.scratch, p, thickness_carve, N));
    DXV_HIP(c, timer_begin(f.timers[kTimerThickness], c->opt.events != 0, fs));
    for (int stage = 0; stage < THICK_STAGES; ++stage) {
        const StageTimer t = stage_timer(c, f, kTimerThickStage0 + stage, c->opt.thickstages, fs);
        DXV_HIP(c, t.begin());
        DXV_HIP(c, launch_thickness_stage(f.grid.p, p, stage, fs));
        DXV_HIP(c, t.end());
    }
    PinnedFrame& pin = cur_pinned(c);
    if (end_operator(c, f, fs, &f.timers[kTimerThickness], pin.thickCount, p.counters, sizeof(pin.thickCount))) return 1;
    f.thick.pending = true;
    f.thick.dim = N; f.thick.cap = cap_sq; f.thick.have = true; f.thick.version = f.gridVersion;
    return 0;
}

int dxv_thickness(dxv_ctx* c, int of, uint32_t cap_sq) { return blocking(c, dxv_thickness_async(c, of, cap_sq)); }

const void* dxv_thickness_device_ptr(const dxv_ctx* c) { return product_ptr(c, "dxv_thickness_device_ptr", kThickMap); }
size_t dxv_thickness_bytes(const dxv_ctx* c) { return product_bytes(c, "dxv_thickness_bytes", kThickMap); }
int dxv_thickness_download(dxv_ctx* c, void* host, size_t bytes) { return product_download(c, "dxv_thickness_download", kThickMap, host, bytes); }
size_t dxv_thickness_histogram_bytes(const dxv_ctx* c) { return product_bytes(c, "dxv_thickness_histogram_bytes", kThickHistogram); }
int dxv_thickness_histogram_download(dxv_ctx* c, void* host, size_t bytes) { return product_download(c, "dxv_thickness_histogram_download", kThickHistogram, host, bytes); }

int dxv_thickness_info(dxv_ctx* c, float* ms, uint64_t* centres_painted, uint64_t* work_items)
{
    if (!c) return 1;
    const Frame& f = cur_frame(c);
    if (ms) *ms = f.timers[kTimerThickness].ms;
    if (centres_painted) *centres_painted = f.thick.centres;
    if (work_items) *work_items = f.thick.items;
    return 0;
}

int dxv_thickness_stage_info(dxv_ctx* c, float ms[6], uint64_t* voxels_tested, uint64_t* atomics_sent)
{
    if (!c) return 1;
    if (!ms) return fail(c, "dxv_thickness_stage_info: ms is NULL");
    const Frame& f = cur_frame(c);
    for (int stage = 0; stage < THICK_STAGES; ++stage) ms[stage] = f.timers[kTimerThickStage0 + stage].ms;
    if (voxels_tested) *voxels_tested = f.thick.tested;
    if (atomics_sent) *atomics_sent = f.thick.sent;
    return 0;
}

// The maximal-ball partition of the selected frame's grid (partition.hip; dxv_partition.h has the rule's routines), enqueued on the frame's stream
// behind whatever it holds, under dxv_render_async's host-wait rule: field, keys, search, roots and their numbering, {K, interface faces} into
// page-locked words and the one wait for them -- the pattern of dxv_components_async: table and sort cannot be sized without them --, then labels
// and table; with throats the faces' words, their sort, T into a page-locked word and a second wait, then the throat records; the frame's end
// event, which nobody waits for here.  Nothing the frame holds is touched before the refusals are through; the product's own buffers are written
// behind the first wait only.  The field of the grid is made into the scratch, never into the frame's distance field.
int dxv_partition_async(dxv_ctx* c, int of, uint32_t cap_sq, int want_throats)
{
    if (!c) return 1;
    if (of != DXV_COMP_SOLID && of != DXV_COMP_EMPTY) return fail(c, "dxv_partition: unknown kind %d (DXV_COMP_SOLID = 0, DXV_COMP_EMPTY = 1)", of);
    if (cap_sq < kPartMinCapSq || cap_sq > kPartMaxCapSq) return fail(c, "dxv_partition: cap_sq %u is not in [%u, %u]", cap_sq, kPartMinCapSq, kPartMaxCapSq);
    if (check_whole_grid(c, "dxv_partition")) return 1;
    Frame& f = cur_frame(c);
    const uint32_t N = f.grid_dim;
    if (N > kThickMaxN) return fail(c, "dxv_partition: a grid of %u^3 voxels; at most %u^3 (a voxel's linear index must fit 30 bits)", N, kThickMaxN);
    hipStream_t fs;
    if (begin_operator(c, &fs)) return 1;
    Frame::Partition& o = f.part;
    const size_t voxels = (size_t)N * N * N, scratch = partition_scratch_bytes(N);
    o.version = 0; o.have = false;
    DXV_HIP(c, o.scratch.reserve(scratch, scratch, fs));
    PartParams p{};
    p.of = of; p.cap = cap_sq; p.prune = (uint32_t)c->opt.partprune; p.count = c->opt.partstages ? 1u : 0u; p.wantThroats = want_throats ? 1u : 0u;
    DXV_HIP(c, carve_buffer(o.scratch, p, partition_carve, N));
    PinnedFrame& pin = cur_pinned(c);
    auto timer_of = [&](int stage) { return stage_timer(c, f, kTimerPartStage0 + stage, c->opt.partstages, fs); };
    DXV_HIP(c, timer_begin(f.timers[kTimerPartition], c->opt.events != 0, fs));
    for (int stage = PART_STAGE_FIELD; stage <= PART_STAGE_ROOTS; ++stage) {
        DXV_HIP(c, timer_of(stage).begin());
        DXV_HIP(c, launch_partition_stage(f.grid.p, p, stage, fs));
        DXV_HIP(c, timer_of(stage).end());
    }
    DXV_HIP(c, hipMemcpyAsync(pin.partTotals, p.totals, sizeof(pin.partTotals), hipMemcpyDeviceToHost, fs));
    DXV_HIP(c, hipStreamSynchronize(fs));
    const uint32_t K = (uint32_t)pin.partTotals[0];
    const unsigned long long faces = want_throats && K ? pin.partTotals[1] : 0ull;
    const size_t work = partition_work_bytes(K, faces);
    DXV_HIP(c, o.labels.reserve(voxels, align256(voxels * sizeof(uint32_t)), fs));
    if (K) DXV_HIP(c, o.table.reserve(K, align256((size_t)K * sizeof(PartRegion)), fs));
    DXV_HIP(c, o.work.reserve(work, work, fs));
    p.labels = o.labels.p; p.table = reinterpret_cast<PartRegion*>(o.table.p);
    DXV_HIP(c, carve_buffer(o.work, p, partition_work_carve, K, faces));
    DXV_HIP(c, timer_of(PART_STAGE_REGIONS).begin());
    DXV_HIP(c, launch_partition_stage(f.grid.p, p, PART_STAGE_REGIONS, fs));
    DXV_HIP(c, timer_of(PART_STAGE_REGIONS).end());
    uint32_t T = 0;
    DXV_HIP(c, timer_of(PART_STAGE_THROATS).begin());
    if (faces) {
        DXV_HIP(c, launch_partition_pairs(p, fs));
        DXV_HIP(c, hipMemcpyAsync(pin.partPairs, p.pairTotal, sizeof(pin.partPairs), hipMemcpyDeviceToHost, fs));
        DXV_HIP(c, hipStreamSynchronize(fs));
        T = (uint32_t)pin.partPairs[0];
        if (T) {
            DXV_HIP(c, o.throats.reserve(T, align256((size_t)T * sizeof(PartThroat)), fs));
            DXV_HIP(c, launch_partition_throats(p, T, o.throats.p, fs));
        }
    }
    DXV_HIP(c, timer_of(PART_STAGE_THROATS).end());
    if (end_operator(c, f, fs, &f.timers[kTimerPartition], pin.partCount, p.counters, sizeof(pin.partCount))) return 1;
    o.pending = true;
    o.dim = N; o.cap = cap_sq; o.of = of; o.hasThroats = want_throats != 0; o.regions = K; o.throatCount = T; o.faces = faces;
    o.have = true; o.version = f.gridVersion;
    return 0;
}

int dxv_partition(dxv_ctx* c, int of, uint32_t cap_sq, int want_throats) { return blocking(c, dxv_partition_async(c, of, cap_sq, want_throats)); }

int dxv_partition_info(dxv_ctx* c, float* ms, uint32_t* regions, uint32_t* throats, uint64_t* interface_faces)
{
    if (!c) return 1;
    const Frame& f = cur_frame(c);
    const bool current = f.part.current(f);
    if (ms) *ms = f.timers[kTimerPartition].ms;
    if (regions) *regions = current ? f.part.regions : 0u;
    if (throats) *throats = current ? f.part.throatCount : 0u;
    if (interface_faces) *interface_faces = current ? f.part.faces : 0u;
    return 0;
}

const void* dxv_partition_labels_device_ptr(const dxv_ctx* c) { return product_ptr(c, "dxv_partition_labels_device_ptr", kPartLabels); }
size_t dxv_partition_labels_bytes(const dxv_ctx* c) { return product_bytes(c, "dxv_partition_labels_bytes", kPartLabels); }
int dxv_partition_labels_download(dxv_ctx* c, void* host, size_t bytes) { return product_download(c, "dxv_partition_labels_download", kPartLabels, host, bytes); }
const void* dxv_partition_table_device_ptr(const dxv_ctx* c) { return product_ptr(c, "dxv_partition_table_device_ptr", kPartTable); }
size_t dxv_partition_table_bytes(const dxv_ctx* c) { return product_bytes(c, "dxv_partition_table_bytes", kPartTable); }
int dxv_partition_table_download(dxv_ctx* c, void* host, size_t bytes) { return product_download(c, "dxv_partition_table_download", kPartTable, host, bytes); }
const void* dxv_partition_throats_device_ptr(const dxv_ctx* c) { return product_ptr(c, "dxv_partition_throats_device_ptr", kPartThroats); }
size_t dxv_partition_throats_bytes(const dxv_ctx* c) { return product_bytes(c, "dxv_partition_throats_bytes", kPartThroats); }
int dxv_partition_throats_download(dxv_ctx* c, void* host, size_t bytes) { return product_download(c, "dxv_partition_throats_download", kPartThroats, host, bytes); }

int dxv_partition_stage_info(dxv_ctx* c, float ms[6], uint64_t* cells_tested, uint64_t* voxels_tested)
{
    if (!c) return 1;
    if (!ms) return fail(c, "dxv_partition_stage_info: ms is NULL");
    const Frame& f = cur_frame(c);
    for (int stage = 0; stage < PART_STAGES; ++stage) ms[stage] = f.timers[kTimerPartStage0 + stage].ms;
    if (cells_tested) *cells_tested = f.part.cellsTested;
    if (voxels_tested) *voxels_tested = f.part.voxelsTested;
    return 0;
}

// The skeleton graph of the selected frame's grid (skeleton.hip; dxv_skeleton.h has the rule's routines), enqueued on the frame's stream behind
// whatever it holds, under dxv_render_async's host-wait rule: pack, classify, init, the components' merge over the node mask and over the curve
// mask, compress and the numbering, {K, B} and the three voxel counts into page-locked words and the one wait for them -- the pattern of
// dxv_components_async: the tables cannot be sized without them --, then the stats kernels and the frame's end event, which nobody waits for here.
// Everything is refused before anything is enqueued or allocated; the grid and the caller's weights are only read.
int dxv_skeleton_async(dxv_ctx* c, const void* device_weights)
{
    if (!c) return 1;
    if (check_whole_grid(c, "dxv_skeleton")) return 1;
    Frame& f = cur_frame(c);
    const uint32_t N = f.grid_dim;
    if (!skel_valid(N)) return fail(c, "dxv_skeleton: a grid of %u^3 voxels; at most %u^3 (bit 31 of a label is its kind)", N, kSkelMaxN);
    const size_t voxels = (size_t)N * N * N;
    DXV_HIP(c, hipSetDevice(c->device));
    if (device_weights) {
        if (reinterpret_cast<uintptr_t>(device_weights) % 4) return fail(c, "dxv_skeleton: weights at %p: need a 4-byte aligned pointer", device_weights);
        size_t room = 0;
        if (const int r = check_device_range(c, "dxv_skeleton", device_weights, voxels * sizeof(uint32_t), &room))
            return r == 1 ? 1 : fail(c, "dxv_skeleton: the weights of %u^3 voxels need %zu bytes, the allocation behind %p has %zu", N, voxels * sizeof(uint32_t), device_weights, room);
    }
    if (settle_frame_launch(c)) return 1;                               // (begin_operator's steps, the device in front of the range check: a pending fill or thin of the frame first)
    const hipStream_t fs = cur_stream(c);
    Frame::Skeleton& o = f.skel;
    const size_t scratch = skel_scratch_bytes(N);
    DXV_HIP(c, o.scratch.reserve(scratch, scratch, fs));
    o.version = 0;                                                      // (the build writes into the frame's label buffer: what it held is gone)
    DXV_HIP(c, o.labels.reserve(voxels, align256(voxels * sizeof(uint32_t)), fs));
    SkelParams p{};
    p.grid = f.grid.p; p.weights = static_cast<const uint32_t*>(device_weights); p.labels = o.labels.p;
    DXV_HIP(c, carve_buffer(o.scratch, p, skel_carve, N));
    unsigned long long* totals = cur_pinned(c).skelTotals;
    DXV_HIP(c, timer_begin(f.timers[kTimerSkeleton], c->opt.events != 0, fs));
    DXV_HIP(c, launch_skel_label(p, fs));
    DXV_HIP(c, hipMemcpyAsync(totals, p.totals, 5 * sizeof(unsigned long long), hipMemcpyDeviceToHost, fs));
    DXV_HIP(c, hipStreamSynchronize(fs));
    const uint32_t K = (uint32_t)totals[0], B = (uint32_t)totals[1];
    if (K | B) {
        if (K) {
            DXV_HIP(c, o.nodes.reserve(K, align256((size_t)K * sizeof(SkelNode)), fs));
            DXV_HIP(c, o.work.reserve((size_t)K * sizeof(SkelNodeStats), align256((size_t)K * sizeof(SkelNodeStats)), fs));
        }
        if (B) DXV_HIP(c, o.branches.reserve(B, align256((size_t)B * sizeof(SkelBranch)), fs));
        p.nodes = reinterpret_cast<SkelNode*>(o.nodes.p);
        p.branches = reinterpret_cast<SkelBranch*>(o.branches.p);
        p.stats = reinterpret_cast<SkelNodeStats*>(o.work.p);
        DXV_HIP(c, launch_skel_stats(p, K, B, fs));
    }
    if (end_operator(c, f, fs, &f.timers[kTimerSkeleton])) return 1;
    o.dim = N; o.nodeCount = K; o.branchCount = B; o.endVoxels = totals[2]; o.curveVoxels = totals[3]; o.junctionVoxels = totals[4];
    o.have = true; o.version = f.gridVersion;
    return 0;
}

int dxv_skeleton(dxv_ctx* c, const void* device_weights) { return blocking(c, dxv_skeleton_async(c, device_weights)); }

int dxv_skeleton_info(dxv_ctx* c, float* ms, uint32_t* nodes, uint32_t* branches, uint64_t* end_voxels, uint64_t* curve_voxels, uint64_t* junction_voxels)
{
    if (!c) return 1;
    const Frame& f = cur_frame(c);
    const bool current = f.skel.current(f);
    if (ms) *ms = f.timers[kTimerSkeleton].ms;
    if (nodes) *nodes = current ? f.skel.nodeCount : 0u;
    if (branches) *branches = current ? f.skel.branchCount : 0u;
    if (end_voxels) *end_voxels = current ? f.skel.endVoxels : 0u;
    if (curve_voxels) *curve_voxels = current ? f.skel.curveVoxels : 0u;
    if (junction_voxels) *junction_voxels = current ? f.skel.junctionVoxels : 0u;
    return 0;
}

const void* dxv_skeleton_labels_device_ptr(const dxv_ctx* c) { return product_ptr(c, "dxv_skeleton_labels_device_ptr", kSkelLabels); }
size_t dxv_skeleton_labels_bytes(const dxv_ctx* c) { return product_bytes(c, "dxv_skeleton_labels_bytes", kSkelLabels); }
int dxv_skeleton_labels_download(dxv_ctx* c, void* host, size_t bytes) { return product_download(c, "dxv_skeleton_labels_download", kSkelLabels, host, bytes); }
const void* dxv_skeleton_nodes_device_ptr(const dxv_ctx* c) { return product_ptr(c, "dxv_skeleton_nodes_device_ptr", kSkelNodes); }
size_t dxv_skeleton_nodes_bytes(const dxv_ctx* c) { return product_bytes(c, "dxv_skeleton_nodes_bytes", kSkelNodes); }
int dxv_skeleton_nodes_download(dxv_ctx* c, void* host, size_t bytes) { return product_download(c, "dxv_skeleton_nodes_download", kSkelNodes, host, bytes); }
const void* dxv_skeleton_branches_device_ptr(const dxv_ctx* c) { return product_ptr(c, "dxv_skeleton_branches_device_ptr", kSkelBranches); }
size_t dxv_skeleton_branches_bytes(const dxv_ctx* c) { return product_bytes(c, "dxv_skeleton_branches_bytes", kSkelBranches); }
int dxv_skeleton_branches_download(dxv_ctx* c, void* host, size_t bytes) { return product_download(c, "dxv_skeleton_branches_download", kSkelBranches, host, bytes); }

// The selected frame's grid edited from its skeleton (skeleton.hip: k_skel_prune_mark; dxv_label.h: k_label_edit), in place, enqueued on the frame's
// stream behind whatever it holds -- under dxv_render_async's host-wait rule and dxv_fill_async's rules for the grid.  Labels and tables are what
// it reads: dxv_trim has left them.  The two counters go into page-locked words and are read where the frame is next synchronised.
int dxv_skeleton_prune_async(dxv_ctx* c, uint32_t max_len345)
{
    if (!c) return 1;
    if (check_current(c, "dxv_skeleton_prune", cur_frame(c).skel, kSkeletonText)) return 1;
    Frame& f = cur_frame(c);
    if (!f.grid.p || f.grid_dim != f.skel.dim || !frame_renderable(f))
        return fail(c, "dxv_skeleton_prune: the skeleton of frame %u does not belong to its grid: it is stale", c->cur);
    hipStream_t fs;
    if (begin_operator(c, &fs)) return 1;
    Frame::Skeleton& o = f.skel;
    const uint32_t K = o.nodeCount, B = o.branchCount;
    const size_t work = skel_prune_bytes(K, B);
    DXV_HIP(c, o.work.reserve(work, work, fs));
    SkelPruneWork w{};
    DXV_HIP(c, carve_buffer(o.work, w, skel_prune_carve, K, B));
    edited_in_place(f);                                                 // (this skeleton is stale with the rest)
    DXV_HIP(c, launch_skel_prune(f.grid.p, o.dim, o.labels.p, reinterpret_cast<const SkelNode*>(o.nodes.p), K, reinterpret_cast<const SkelBranch*>(o.branches.p), B, max_len345, w,
                                 fs));
    PinnedFrame& pin = cur_pinned(c);
    if (end_operator(c, f, fs, nullptr, pin.skelPrune, w.counters, sizeof(pin.skelPrune))) return 1;
    o.prune.pending = true;
    return 0;
}

int dxv_skeleton_prune(dxv_ctx* c, uint32_t max_len345) { return blocking(c, dxv_skeleton_prune_async(c, max_len345)); }

int dxv_skeleton_prune_info(dxv_ctx* c, uint32_t* branches_removed, uint64_t* voxels_removed)
{
    if (!c) return 1;
    const Frame& f = cur_frame(c);
    if (branches_removed) *branches_removed = f.skel.prune.branches;
    if (voxels_removed) *voxels_removed = f.skel.prune.voxels;
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
    if (check_seed_args(c, "dxv_geodesic", seeds_kind, seeds, seed_count)) return 1;
    if (check_whole_grid(c, "dxv_geodesic")) return 1;
    Frame& f = cur_frame(c);
    const uint32_t N = f.grid_dim;
    if (N > kGeoMaxN) return fail(c, "dxv_geodesic: a grid of %u^3 voxels; at most %u^3", N, kGeoMaxN);
    if (!geo_fits(N, metric))
        return fail(c, "dxv_geodesic: a grid of %u^3 voxels under metric %d: a path of weight %u per step can reach the codes of the map (wmax (N^3 - 1) must stay below 0xFFFFFFFE)", N,
                    metric, geo_max_weight(metric));
    hipStream_t fs;
    if (begin_seeded(c, "dxv_geodesic", seeds_kind, seeds, seed_count, N, &fs)) return 1;
    const size_t voxels = cube(N), scratch = geodesic_scratch_bytes(N);
    f.geo.version = 0; f.geo.have = false;
    DXV_HIP(c, f.geo.map.reserve(voxels, align256(voxels * sizeof(uint32_t)), fs));
    DXV_HIP(c, f.geo.scratch.reserve(scratch, scratch, fs));
    GeoScratch l{};
    DXV_HIP(c, carve_buffer(f.geo.scratch, l, geodesic_carve, N));
    const void* deviceSeeds;
    if (upload_seeds(c, f.geo, seeds_kind, seeds, seed_count, fs, &deviceSeeds)) return 1;
    f.geo.metric = metric; f.geo.limit = limit;
    begin_flood(f.geo, c->opt.georounds, kGeoRoundsDefault);
    DXV_HIP(c, timer_begin(f.timers[kTimerGeodesic], c->opt.events != 0, fs));
    DXV_HIP(c, launch_geodesic_init(f.grid.p, N, of, seeds_kind, deviceSeeds, seed_count, f.geo.map.p, l, fs));
    DXV_HIP(c, launch_geodesic_batch(f.geo.map.p, N, metric, limit, l, f.geo.batch, 0u, fs));
    if (end_operator(c, f, fs, &f.timers[kTimerGeodesic], &cur_pinned(c).geoCtl, l.ctl, sizeof(GeoControl))) return 1;
    f.geo.pending = true;
    f.geo.dim = N; f.geo.have = true; f.geo.version = f.gridVersion;
    return 0;
}

int dxv_geodesic(dxv_ctx* c, int of, int metric, int seeds_kind, const void* seeds, uint32_t seed_count, uint32_t limit) { return blocking(c, dxv_geodesic_async(c, of, metric, seeds_kind, seeds, seed_count, limit)); }

const void* dxv_geodesic_device_ptr(const dxv_ctx* c) { return product_ptr(c, "dxv_geodesic_device_ptr", kGeoMap); }
size_t dxv_geodesic_bytes(const dxv_ctx* c) { return product_bytes(c, "dxv_geodesic_bytes", kGeoMap); }
int dxv_geodesic_download(dxv_ctx* c, void* host, size_t bytes) { return product_download(c, "dxv_geodesic_download", kGeoMap, host, bytes); }

int dxv_geodesic_info(dxv_ctx* c, float* ms, uint32_t* rounds, uint64_t* seeds_used, uint64_t* reached, uint64_t* unreached, uint32_t* farthest, uint32_t* farthest_voxel)
{
    if (!c || check_current(c, "dxv_geodesic_info", cur_frame(c).geo, kGeodesicText)) return 1;
    const Frame& f = cur_frame(c);
    if (ms) *ms = f.timers[kTimerGeodesic].ms;
    if (rounds) *rounds = f.geo.rounds;
    if (seeds_used) *seeds_used = f.geo.seedsUsed;
    if (reached) *reached = f.geo.reached;
    if (unreached) *unreached = f.geo.unreached;
    if (farthest) *farthest = f.geo.farthest;
    if (farthest_voxel) *farthest_voxel = f.geo.farthestVoxel;
    return 0;
}

int dxv_geodesic_work_info(dxv_ctx* c, uint64_t* tiles_run, uint32_t* most_live_tiles, uint32_t* sparse_rounds)
{
    return c ? flood_work_info(c, "dxv_geodesic_work_info", cur_frame(c).geo, kGeodesicText, tiles_run, most_live_tiles, sparse_rounds) : 1;
}

// The access radius inside the selected frame's grid and its intrusion map (access.hip; dxv_access.h has the rule's routines), enqueued on the
// frame's stream behind whatever it holds, under dxv_render_async's host-wait rule and the geodesic's discipline: the radius field, the init,
// ONE batch of rounds, the tally, the batch's control block into page-locked words, the frame's end event.  Whether the batch reached the fixed
// point is read where the frame is next synchronised (settle_access), which also makes the intrusion map and the histograms behind the last
// batch.  Everything is refused before anything is enqueued or allocated; the grid is only read.
int dxv_access_async(dxv_ctx* c, int of, int connectivity, uint32_t cap_sq, int seeds_kind, const void* seeds, uint32_t seed_count, int want_intrusion)
{
    if (!c) return 1;
    if (of != DXV_COMP_SOLID && of != DXV_COMP_EMPTY) return fail(c, "dxv_access: unknown kind %d (DXV_COMP_SOLID = 0, DXV_COMP_EMPTY = 1)", of);
    if (!acc_connectivity(connectivity)) return fail(c, "dxv_access: connectivity %d is neither 6 nor 26", connectivity);
    if (cap_sq < kThickMinCapSq || cap_sq > kThickMaxCapSq) return fail(c, "dxv_access: cap_sq %u is not in [%u, %u]", cap_sq, kThickMinCapSq, kThickMaxCapSq);
    if (check_seed_args(c, "dxv_access", seeds_kind, seeds, seed_count)) return 1;
    if (check_whole_grid(c, "dxv_access")) return 1;
    Frame& f = cur_frame(c);
    const uint32_t N = f.grid_dim;
    if (N > kAccMaxN) return fail(c, "dxv_access: a grid of %u^3 voxels; at most %u^3 (a centre's linear index must fit 30 bits)", N, kAccMaxN);
    hipStream_t fs;
    if (begin_seeded(c, "dxv_access", seeds_kind, seeds, seed_count, N, &fs)) return 1;
    Frame::Access& o = f.acc;
    const bool intrusion = want_intrusion != 0;
    const size_t voxels = cube(N), scratch = access_scratch_bytes(N, intrusion);
    o.version = 0; o.have = false;
    DXV_HIP(c, o.map.reserve(voxels, align256(voxels * sizeof(uint32_t)), fs));
    DXV_HIP(c, o.hist.reserve(kThickMaxCapSq + 1u, align256(thickness_histogram_bytes(kThickMaxCapSq)), fs));
    if (intrusion) {
        DXV_HIP(c, o.intrusion.reserve(voxels, align256(voxels * sizeof(uint32_t)), fs));
        DXV_HIP(c, o.histI.reserve(kThickMaxCapSq + 1u, align256(thickness_histogram_bytes(kThickMaxCapSq)), fs));
    }
    DXV_HIP(c, o.scratch.reserve(scratch, scratch, fs));
    AccScratch l{};
    DXV_HIP(c, carve_buffer(o.scratch, l, access_carve, N, intrusion));
    const void* deviceSeeds;
    if (upload_seeds(c, o, seeds_kind, seeds, seed_count, fs, &deviceSeeds)) return 1;
    o.dim = N; o.cap = cap_sq; o.of = of; o.connectivity = connectivity; o.wantIntrusion = intrusion; o.cull = (uint32_t)c->opt.thickcull;
    begin_flood(o, c->opt.accessrounds, kAccRoundsDefault);
    DXV_HIP(c, timer_begin(f.timers[kTimerAccess], c->opt.events != 0, fs));
    DXV_HIP(c, launch_access_init(f.grid.p, N, of, cap_sq, seeds_kind, deviceSeeds, seed_count, o.map.p, l, fs));
    DXV_HIP(c, launch_access_batch(o.map.p, N, of, connectivity, cap_sq, l, o.batch, 0u, fs));
    if (end_operator(c, f, fs, &f.timers[kTimerAccess], &cur_pinned(c).accCtl, l.ctl, sizeof(GeoControl))) return 1;
    o.pending = true;
    o.have = true; o.version = f.gridVersion;
    return 0;
}

int dxv_access(dxv_ctx* c, int of, int connectivity, uint32_t cap_sq, int seeds_kind, const void* seeds, uint32_t seed_count, int want_intrusion)
{
    return blocking(c, dxv_access_async(c, of, connectivity, cap_sq, seeds_kind, seeds, seed_count, want_intrusion));
}

const void* dxv_access_device_ptr(const dxv_ctx* c) { return product_ptr(c, "dxv_access_device_ptr", kAccMap); }
size_t dxv_access_bytes(const dxv_ctx* c) { return product_bytes(c, "dxv_access_bytes", kAccMap); }
int dxv_access_download(dxv_ctx* c, void* host, size_t bytes) { return product_download(c, "dxv_access_download", kAccMap, host, bytes); }
size_t dxv_access_histogram_bytes(const dxv_ctx* c) { return product_bytes(c, "dxv_access_histogram_bytes", kAccHistogram); }
int dxv_access_histogram_download(dxv_ctx* c, void* host, size_t bytes) { return product_download(c, "dxv_access_histogram_download", kAccHistogram, host, bytes); }
// (the intrusion map's: the access map's refusals, and one more for a map made without it)
const void* dxv_intrusion_device_ptr(const dxv_ctx* c) { return product_ptr(c, "dxv_intrusion_device_ptr", kIntrusionMap); }
size_t dxv_intrusion_bytes(const dxv_ctx* c) { return product_bytes(c, "dxv_intrusion_bytes", kIntrusionMap); }
int dxv_intrusion_download(dxv_ctx* c, void* host, size_t bytes) { return product_download(c, "dxv_intrusion_download", kIntrusionMap, host, bytes); }
size_t dxv_intrusion_histogram_bytes(const dxv_ctx* c) { return product_bytes(c, "dxv_intrusion_histogram_bytes", kIntrusionHistogram); }
int dxv_intrusion_histogram_download(dxv_ctx* c, void* host, size_t bytes) { return product_download(c, "dxv_intrusion_histogram_download", kIntrusionHistogram, host, bytes); }

int dxv_access_info(dxv_ctx* c, float* ms, uint32_t* rounds, uint64_t* seeds_used, uint64_t* reached, uint64_t* unreached, uint32_t* widest, uint32_t* widest_voxel)
{
    if (!c || check_current(c, "dxv_access_info", cur_frame(c).acc, kAccessText)) return 1;
    const Frame& f = cur_frame(c);
    if (ms) *ms = f.timers[kTimerAccess].ms;
    if (rounds) *rounds = f.acc.rounds;
    if (seeds_used) *seeds_used = f.acc.seedsUsed;
    if (reached) *reached = f.acc.reached;
    if (unreached) *unreached = f.acc.unreached;
    if (widest) *widest = f.acc.widest;
    if (widest_voxel) *widest_voxel = f.acc.widestVoxel;
    return 0;
}

int dxv_access_work_info(dxv_ctx* c, uint64_t* tiles_run, uint32_t* most_live_tiles, uint32_t* sparse_rounds)
{
    return c ? flood_work_info(c, "dxv_access_work_info", cur_frame(c).acc, kAccessText, tiles_run, most_live_tiles, sparse_rounds) : 1;
}

// The line-of-sight map of the selected frame's grid (sight.hip; dxv_sight.h has the rule's routines), enqueued on the frame's stream behind
// whatever it holds, under dxv_render_async's host-wait rule.  A fixed chain of kernels: nothing to settle; the tally goes into page-locked
// words and is read where the frame is next synchronised.  Map and scratch are the frame's own.
int dxv_sight_async(dxv_ctx* c, int of, uint32_t directions)
{
    if (!c) return 1;
    if (of != DXV_COMP_SOLID && of != DXV_COMP_EMPTY) return fail(c, "dxv_sight: unknown kind %d (DXV_COMP_SOLID = 0, DXV_COMP_EMPTY = 1)", of);
    if (!sight_directions_valid(directions))
        return fail(c, "dxv_sight: directions 0x%08X is not a non-empty subset of DXV_SIGHT_ALL = 0x%08X (bit 13 is the zero vector, bits 27 .. 31 are none)", directions, kSightAll);
    if (check_whole_grid(c, "dxv_sight")) return 1;
    Frame& f = cur_frame(c);
    const uint32_t N = f.grid_dim;
    if (N > kSightMaxN) return fail(c, "dxv_sight: a grid of %u^3 voxels; at most %u^3 (a voxel's linear index must fit 30 bits)", N, kSightMaxN);
    hipStream_t fs;
    if (begin_operator(c, &fs)) return 1;
    Frame::Sight& o = f.sight;
    const size_t voxels = cube(N), scratch = sight_scratch_bytes(N, directions);
    o.version = 0; o.have = false;
    DXV_HIP(c, o.map.reserve(voxels, align256(voxels * sizeof(uint32_t)), fs));
    DXV_HIP(c, o.scratch.reserve(scratch, scratch, fs));
    SightScratch l{};
    DXV_HIP(c, carve_buffer(o.scratch, l, sight_carve, N, directions));
    DXV_HIP(c, timer_begin(f.timers[kTimerSight], c->opt.events != 0, fs));
    DXV_HIP(c, launch_sight(f.grid.p, N, of, directions, (uint32_t)c->opt.sightgroup, o.map.p, l, fs));
    PinnedFrame& pin = cur_pinned(c);
    if (end_operator(c, f, fs, &f.timers[kTimerSight], pin.sightTally, l.tally, sizeof(pin.sightTally))) return 1;
    o.pending = true;
    o.dim = N; o.of = of; o.directions = directions; o.have = true; o.version = f.gridVersion;
    return 0;
}

int dxv_sight(dxv_ctx* c, int of, uint32_t directions) { return blocking(c, dxv_sight_async(c, of, directions)); }

const void* dxv_sight_device_ptr(const dxv_ctx* c) { return product_ptr(c, "dxv_sight_device_ptr", kSightMap); }
size_t dxv_sight_bytes(const dxv_ctx* c) { return product_bytes(c, "dxv_sight_bytes", kSightMap); }
int dxv_sight_download(dxv_ctx* c, void* host, size_t bytes) { return product_download(c, "dxv_sight_download", kSightMap, host, bytes); }

// (the tally is the host's by the time the frame has been synchronised: the map's refusals, the byte count, the synchronisation, a copy)
int dxv_sight_tally_download(dxv_ctx* c, void* host, size_t bytes)
{
    if (!c || check_current(c, "dxv_sight_tally_download", cur_frame(c).sight, kSightText)) return 1;
    const size_t want = sizeof(cur_frame(c).sight.tally);
    if (!host || bytes != want) return fail(c, "dxv_sight_tally_download: expected %zu bytes, got %zu", want, bytes);
    if (dxv_sync(c)) return 1;
    memcpy(host, cur_frame(c).sight.tally, want);
    return 0;
}

int dxv_sight_info(dxv_ctx* c, float* ms, int* of, uint32_t* directions)
{
    if (!c || check_current(c, "dxv_sight_info", cur_frame(c).sight, kSightText)) return 1;
    const Frame& f = cur_frame(c);
    if (ms) *ms = f.timers[kTimerSight].ms;
    if (of) *of = f.sight.of;
    if (directions) *directions = f.sight.directions;
    return 0;
}

// The selected frame's grid edited from its line-of-sight map (sight.hip: k_sight_fill), in place, enqueued on the frame's stream behind whatever
// it holds -- under dxv_render_async's host-wait rule and dxv_fill_async's rules for the grid.  The map is what it reads: dxv_trim has left it.
int dxv_sight_fill_async(dxv_ctx* c, uint32_t directions)
{
    if (!c) return 1;
    if (check_current(c, "dxv_sight_fill", cur_frame(c).sight, kSightText)) return 1;
    Frame& f = cur_frame(c);
    Frame::Sight& o = f.sight;
    if (!directions || (directions & ~o.directions))
        return fail(c, "dxv_sight_fill: directions 0x%08X is not a non-empty subset of the 0x%08X the map of frame %u was made with", directions, o.directions, c->cur);
    if (!f.grid.p || f.grid_dim != o.dim || !frame_renderable(f))
        return fail(c, "dxv_sight_fill: the line-of-sight map of frame %u does not belong to its grid: it is stale", c->cur);
    hipStream_t fs;
    if (begin_operator(c, &fs)) return 1;
    edited_in_place(f);                                                 // (this map is stale with the rest)
    DXV_HIP(c, launch_sight_fill(f.grid.p, o.dim, o.of, directions, o.map.p, fs));
    return end_operator(c, f, fs, nullptr);
}

int dxv_sight_fill(dxv_ctx* c, uint32_t directions) { return blocking(c, dxv_sight_fill_async(c, directions)); }

// The path from `target` down to a seed of the selected frame's current map, synchronous: the frame is synchronised, the target's word is read,
// one wave walks down (geodesic.hip: k_geo_path) into the frame's own words, and min(length, capacity) of them come back.
int dxv_geodesic_path(dxv_ctx* c, uint32_t target, uint32_t* host_path, uint32_t capacity, uint32_t* length)
{
    if (!c || check_current(c, "dxv_geodesic_path", cur_frame(c).geo, kGeodesicText)) return 1;
    if (!length) return fail(c, "dxv_geodesic_path: length is NULL");
    if (capacity && !host_path) return fail(c, "dxv_geodesic_path: room for %u voxels at NULL", capacity);
    Frame& f = cur_frame(c);
    const uint32_t N = f.geo.dim;
    const size_t voxels = (size_t)N * N * N;
    if (target >= voxels) return fail(c, "dxv_geodesic_path: target %u is outside the grid of %u^3 = %zu voxels", target, N, voxels);
    if (dxv_sync(c)) return 1;
    const hipStream_t fs = cur_stream(c);
    uint32_t word = 0;
    DXV_HIP(c, hipMemcpyAsync(&word, f.geo.map.p + target, sizeof(word), hipMemcpyDeviceToHost, fs));
    DXV_HIP(c, hipStreamSynchronize(fs));
    if (word >= kGeoUnreached)
        return fail(c, "dxv_geodesic_path: target %u holds no distance (%s)", target, word == kGeoNone ? "DXV_GEO_NONE: it is no member" : "DXV_GEO_UNREACHED: no path reaches it");
    const uint64_t longest = (uint64_t)word / geo_min_weight(f.geo.metric) + 1u;     // (every step lowers the word by the least weight or more)
    const uint32_t room = (uint64_t)capacity < longest ? capacity : (uint32_t)longest;
    DXV_HIP(c, f.geo.path.reserve((size_t)room + 2u, align256(((size_t)room + 2u) * sizeof(uint32_t)), fs));
    DXV_HIP(c, launch_geodesic_path(f.geo.map.p, N, f.geo.metric, target, f.geo.path.p, room, fs));
    uint32_t head[2] = {0, 0};
    DXV_HIP(c, hipMemcpyAsync(head, f.geo.path.p, sizeof(head), hipMemcpyDeviceToHost, fs));
    DXV_HIP(c, hipStreamSynchronize(fs));
    if (head[1] || head[0] > longest) return fail(c, "dxv_geodesic_path: no neighbour continues the path after %u voxels from target %u: the map is no fixed point", head[0], target);
    *length = head[0];
    const uint32_t give = head[0] < room ? head[0] : room;
    if (give) {
        DXV_HIP(c, hipMemcpyAsync(host_path, f.geo.path.p + 2, (size_t)give * sizeof(uint32_t), hipMemcpyDeviceToHost, fs));
        DXV_HIP(c, hipStreamSynchronize(fs));
    }
    return 0;
}

// The selected frame's grid edited from its labels (components.hip: k_comp_keep; dxv_label.h: k_label_edit), in place, enqueued on the frame's stream behind
// whatever it holds -- under dxv_render_async's host-wait rule and dxv_fill_async's rules for the grid.  The four counters go into page-locked
// words and are read where the frame is next synchronised.
int dxv_components_select_async(dxv_ctx* c, int rule, uint32_t arg)
{
    if (!c) return 1;
    if (rule != DXV_SELECT_LARGEST && rule != DXV_SELECT_MIN_VOXELS && rule != DXV_SELECT_BORDER)
        return fail(c, "dxv_components_select: unknown rule %d (DXV_SELECT_LARGEST = 0, DXV_SELECT_MIN_VOXELS = 1, DXV_SELECT_BORDER = 2)", rule);
    if (rule != DXV_SELECT_MIN_VOXELS && arg) return fail(c, "dxv_components_select: rule %d takes no argument (arg must be 0, got %u)", rule, arg);
    if (check_current(c, "dxv_components_select", cur_frame(c).comp, kComponentsText)) return 1;
    Frame& f = cur_frame(c);
    if (!f.grid.p || f.grid_dim != f.comp.dim || !frame_renderable(f))
        return fail(c, "dxv_components_select: the labels of frame %u do not belong to its grid: they are stale", c->cur);
    hipStream_t fs;
    if (begin_operator(c, &fs)) return 1;
    const uint32_t K = f.comp.count;
    const size_t work = comp_select_bytes(K);
    DXV_HIP(c, f.comp.work.reserve(work, work, fs));
    CompSelectWork w{};
    DXV_HIP(c, carve_buffer(f.comp.work, w, comp_select_carve, K));
    edited_in_place(f);                                                 // (these labels are stale with the rest)
    DXV_HIP(c, launch_comp_select(f.grid.p, f.comp.dim, f.comp.of, f.comp.labels.p, reinterpret_cast<const CompRecord*>(f.comp.table.p), K, rule, arg, w, fs));
    PinnedFrame& pin = cur_pinned(c);
    if (end_operator(c, f, fs, nullptr, pin.compSel, w.counters, sizeof(pin.compSel))) return 1;
    f.comp.select.pending = true; f.comp.select.rule = rule; f.comp.select.components = K;
    return 0;
}

int dxv_components_select(dxv_ctx* c, int rule, uint32_t arg) { return blocking(c, dxv_components_select_async(c, rule, arg)); }

int dxv_components_select_info(dxv_ctx* c, uint32_t* kept, uint32_t* dropped, uint64_t* voxels_changed)
{
    if (!c) return 1;
    const Frame& f = cur_frame(c);
    if (kept) *kept = f.comp.select.kept;
    if (dropped) *dropped = f.comp.select.dropped;
    if (voxels_changed) *voxels_changed = f.comp.select.changed;
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
    hipStream_t fs;
    if (begin_operator(c, &fs)) return 1;
    const uint32_t N = f.grid_dim;
    const size_t scratch = fill_scratch_bytes(N);
    DXV_HIP(c, f.fill.scratch.reserve(scratch, scratch, fs));
    FillScratch l{};
    DXV_HIP(c, carve_buffer(f.fill.scratch, l, fill_carve, N));
    f.fill.what = what;
    f.fill.batch = c->opt.fillrounds ? (uint32_t)c->opt.fillrounds : kFillRoundsDefault;
    f.fill.rounds = 0;
    edited_in_place(f);
    DXV_HIP(c, timer_begin(f.timers[kTimerFill], c->opt.events != 0, fs));
    DXV_HIP(c, launch_fill(f.grid.p, N, what, l, f.fill.batch, true, fs));
    PinnedFrame& pin = cur_pinned(c);
    if (end_operator(c, f, fs, &f.timers[kTimerFill], pin.fillCtl, l.ctl, sizeof(pin.fillCtl))) return 1;
    f.fill.pending = true;
    return 0;
}

int dxv_fill(dxv_ctx* c, int what) { return blocking(c, dxv_fill_async(c, what)); }

int dxv_fill_info(dxv_ctx* c, float* ms, uint32_t* rounds)
{
    if (!c) return 1;
    if (ms) *ms = cur_frame(c).timers[kTimerFill].ms;
    if (rounds) *rounds = cur_frame(c).fill.rounds;
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
    hipStream_t fs;
    if (begin_operator(c, &fs)) return 1;
    const uint32_t N = f.grid_dim;
    const int form = morph_form(radius_sq, c->opt.morphform);
    const size_t scratch = morph_scratch_bytes(N, op, radius_sq, form);
    DXV_HIP(c, f.morph.scratch.reserve(scratch, scratch, fs));
    MorphScratch l{};
    DXV_HIP(c, carve_buffer(f.morph.scratch, l, morph_carve, N, op, radius_sq, form));
    edited_in_place(f);
    DXV_HIP(c, timer_begin(f.timers[kTimerMorph], c->opt.events != 0, fs));
    DXV_HIP(c, launch_morph(f.grid.p, N, op, radius_sq, form, l, fs));
    PinnedFrame& pin = cur_pinned(c);
    if (end_operator(c, f, fs, &f.timers[kTimerMorph], pin.morphCount, l.counters, sizeof(pin.morphCount))) return 1;
    f.morph.pending = true;
    return 0;
}

int dxv_morph(dxv_ctx* c, int op, uint32_t radius_sq) { return blocking(c, dxv_morph_async(c, op, radius_sq)); }

int dxv_morph_info(dxv_ctx* c, float* ms, uint64_t* voxels_set, uint64_t* voxels_cleared)
{
    if (!c) return 1;
    const Frame& f = cur_frame(c);
    if (ms) *ms = f.timers[kTimerMorph].ms;
    if (voxels_set) *voxels_set = f.morph.set;
    if (voxels_cleared) *voxels_cleared = f.morph.cleared;
    return 0;
}

// Topology-preserving thinning of the selected frame's grid (thin.hip), in place, enqueued on the frame's stream behind whatever it holds -- under
// dxv_render_async's host-wait rule and dxv_fill_async's rules for the grid: one batch of iterations, the write-back, the batch's control block
// into page-locked words, the frame's end event.  Whether the batch reached the fixed point is read where the frame is next synchronised
// (settle_thin).  Everything is refused before anything is enqueued or waited for.
int dxv_thin_async(dxv_ctx* c, int kind, uint32_t max_iterations)
{
    if (!c) return 1;
    if (kind != DXV_THIN_CURVE && kind != DXV_THIN_KERNEL)
        return fail(c, "dxv_thin: unknown kind %d (DXV_THIN_CURVE = 0, DXV_THIN_KERNEL = 1)", kind);
    if (check_whole_grid(c, "dxv_thin")) return 1;
    Frame& f = cur_frame(c);
    const uint32_t N = f.grid_dim;
    if (N > kThinMaxN || (N & 1u)) return fail(c, "dxv_thin: a grid of side %u (needs an even side of at most %u)", N, kThinMaxN);
    hipStream_t fs;
    if (begin_operator(c, &fs)) return 1;
    const size_t scratch = thin_scratch_bytes(N);
    DXV_HIP(c, f.thin.scratch.reserve(scratch, scratch, fs));
    ThinScratch l{};
    DXV_HIP(c, carve_buffer(f.thin.scratch, l, thin_carve, N));
    f.thin.kind = kind;
    f.thin.batch = c->opt.thinrounds ? (uint32_t)c->opt.thinrounds : kThinRoundsDefault;
    f.thin.bounded = max_iterations != 0u;
    f.thin.inBatch = thin_batch(f.thin.batch, max_iterations);
    f.thin.left = f.thin.bounded ? max_iterations - f.thin.inBatch : 0u;
    f.thin.iterations = 0;
    f.thin.removed = 0;
    f.thin.converged = false;
    edited_in_place(f);
    DXV_HIP(c, timer_begin(f.timers[kTimerThin], c->opt.events != 0, fs));
    DXV_HIP(c, launch_thin(f.grid.p, N, kind, l, f.thin.inBatch, true, fs));
    if (end_operator(c, f, fs, &f.timers[kTimerThin], &cur_pinned(c).thinCtl, l.ctl, sizeof(ThinControl))) return 1;
    f.thin.pending = true;
    return 0;
}

int dxv_thin(dxv_ctx* c, int kind, uint32_t max_iterations) { return blocking(c, dxv_thin_async(c, kind, max_iterations)); }

int dxv_thin_info(dxv_ctx* c, float* ms, uint32_t* iterations, uint64_t* voxels_removed, int* converged)
{
    if (!c) return 1;
    const Frame& f = cur_frame(c);
    if (ms) *ms = f.timers[kTimerThin].ms;
    if (iterations) *iterations = f.thin.iterations;
    if (voxels_removed) *voxels_removed = f.thin.removed;
    if (converged) *converged = f.thin.converged ? 1 : 0;
    return 0;
}
} // extern "C"
