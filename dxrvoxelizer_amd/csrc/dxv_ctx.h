// dxv_ctx.h -- the context of libdxv.so and what its translation units share: dxv_api.hip (context, mesh, build, options,
// results), dxv_lists.hip (the candidate lists' policy and builds), dxv_frames.hip (frames, launches, work queues),
// dxv_products.hip (what is made of a frame's grid and what edits it in place: one record of Frame per operator), dxv_blob.hip (the
// scene blob that travels between GPUs), dxv_debug.hip (test hooks).  Nothing here is exported.
#pragma once
#include "../../include/dxv.h"
#include "dxv_device.h"
#include "dxv_raycast.h"
#include "dxv_dirmap.h"
#include "dxv_policy.h"
#include "dxv_geodesic.h"       // GeoControl and ThinControl, which the page-locked words of a frame hold whole
#include "dxv_thin.h"

#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <algorithm>
#include <atomic>
#include <string>
#include <thread>
#include <vector>

namespace dxvhost {
#if defined(DXV_QUEUE_TIMES)
constexpr uint32_t kRedoCap = 1u << 21;   // (diagnostic build: the list doubles as the buffer of per-workgroup time stamps)
#else
constexpr uint32_t kRedoCap = 1u << 16;   // rays per launch the redo pass takes before the column is grown instead
#endif
constexpr uint32_t kOctStatusWord = 3;    // the word of a frame's status block an octree expansion raises (words 0 .. 2 are the launch's)
}

using namespace dxv;
using dxvhost::kRedoCap;
using dxvhost::kOctStatusWord;

// A device allocation together with the capacity it was made for.  The two cannot disagree (p is null exactly when cap is 0), the
// memory is freed exactly once (release, or the end of the owner) and the value moves but does not copy -- so nothing that owns
// one has to be named again where the context is trimmed or destroyed.  `cap` counts in the owner's unit (elements, words, bytes,
// texels per side): reserve is told both what to record and how many bytes to allocate for it, because several owners allocate
// spare room behind what they count.
template <class T> struct DevBuf {
    T* p = nullptr;
    size_t cap = 0;
    DevBuf() = default;
    DevBuf(const DevBuf&) = delete;
    DevBuf& operator=(const DevBuf&) = delete;
    DevBuf(DevBuf&& o) noexcept : p(o.p), cap(o.cap) { o.p = nullptr; o.cap = 0; }
    DevBuf& operator=(DevBuf&& o) noexcept
    {
        if (this != &o) { release(); p = o.p; cap = o.cap; o.p = nullptr; o.cap = 0; }
        return *this;
    }
    ~DevBuf() { release(); }
    void release()
    {
        if (p) (void)hipFree(p);
        p = nullptr; cap = 0;
    }
    // grow only: reallocates when need > cap, never shrinks.  A failed allocation leaves the buffer empty.
    hipError_t reserve(size_t need, size_t bytes)
    {
        if (need <= cap) return hipSuccess;
        release();
        const hipError_t e = hipMalloc(reinterpret_cast<void**>(&p), bytes);
        if (e == hipSuccess) cap = need; else p = nullptr;
        return e;
    }
    // ... for memory a stream may still be using: that stream is waited for in front of the free
    hipError_t reserve(size_t need, size_t bytes, hipStream_t user)
    {
        if (need <= cap) return hipSuccess;
        const hipError_t e = hipStreamSynchronize(user);
        return e != hipSuccess ? e : reserve(need, bytes);
    }
    // grow, or give back when oversized: reallocates when need > cap or cap > 2 * need (a scene or mesh of about the size of
    // the last one moves into its allocation: a free and an allocation of a hundred megabytes less on the way to the first launch)
    hipError_t fit(size_t bytes)
    {
        if (cap > 2 * bytes) release();
        return reserve(bytes, bytes);
    }
};

// direction-space lists of the reference rule (dxv_dirmap.h), built lazily from the scene's triangle records, with the max-mip of
// their far radii: made with the lists, what a launch's work queue is probed against
struct Lists {
    DevBuf<DirCell> cells;
    DevBuf<DirEntry> entries;
    DevBuf<uint16_t> mip;            // (cap: 16-bit words of the mip proper)
    DevBuf<uint32_t> starts;         // start table (dxv_dirmap.h: dm_start_word): one word per texel, made with the mip wherever cells and entries are; two counters behind it
    DevBuf<DirCell> startCells;      // start cells (dxv_dirmap.h: dm_start_cell): the cells with the table's word where the hints are, made with the table by dirmap_starts; never exported
    bool startsPay = false;          // what option starttable = 2 (automatic) does for these lists (dxv_policy.h: start_table_pays; false until the build is settled)
    uint32_t count = 0, res = 0;     // entries, texels per face side
    int state = 0;                   // 0: not built for this scene, 1: built, -1: over the cap for this scene (tree walk)
    int opt = 0;                     // the listres option these lists (or the decision against them) were made with
    float ms = 0.0f;
    // room for lists of n entries on map R (+ spare entries: a scan round loads four; the mip buffer: far radii, entry counts)
    hipError_t reserve(uint32_t R, size_t n)
    {
        hipError_t e = cells.reserve(6 * (size_t)R * R, 6 * (size_t)R * R * sizeof(DirCell));
        if (e == hipSuccess) e = entries.reserve(n, (n + 4) * sizeof(DirEntry));
        if (e == hipSuccess) e = mip.reserve(dm_mip_words(R), sizeof(uint16_t) * (size_t)dm_mip_buffer_words(R));
        if (e == hipSuccess) e = starts.reserve(6 * (size_t)R * R + 2, (6 * (size_t)R * R + 2) * sizeof(uint32_t));
        if (e == hipSuccess) e = startCells.reserve(6 * (size_t)R * R, 6 * (size_t)R * R * sizeof(DirCell));
        return e;
    }
};
// row lists of the parity rule (parity_lists.hip): built like the direction-space lists, on a scene's second parity launch or on
// a large first one; an importing context adopts the ones in the blob or builds its own from the triangle records (0.2 ms)
struct RowLists {
    DevBuf<uint32_t> cells, entries;
    DevBuf<uint32_t> scratch;        // counts, offsets, block sums of the build
    uint32_t count = 0, res = 0;
    int state = 0;                   // 0: not built for this scene, 1: built, -1: over the cap (tree walk)
    float ms = 0.0f;
    // room for row lists of n entries on an R x R grid (the kernel fetches up to three slots behind the end of a list: spare words)
    hipError_t reserve(uint32_t R, size_t n)
    {
        const hipError_t e = cells.reserve(2 * (size_t)R * R, 2 * (size_t)R * R * sizeof(uint32_t));
        return e != hipSuccess ? e : entries.reserve(n + 8, (n + 8) * sizeof(uint32_t));
    }
};
// far-radius map of a scene WITHOUT lists (dirmap_far): the brick test of its tree walks; made at the scene's first tree walk
struct FarMap {
    DevBuf<uint32_t> far32;          // (cap of the three: the map side they were allocated for)
    DevBuf<DirCell> cells;
    DevBuf<uint16_t> mip;
    uint32_t R = 0;                  // the map it is on
    uint64_t epoch = 0;              // the scene epoch it was made for (0: none)
    float ms = 0.0f;
};
// build scratch (dxv_build; dxv_refit reads keys and links again)
struct BuildScratch {
    DevBuf<uint64_t> keys, keysTmp;  // (cap of keys: the triangles the scratch was allocated for -- alloc_scratch keeps it for meshes of half to all of that)
    DevBuf<uint32_t> hist, parents, flags, flags2;   // (cap of hist: words)
    DevBuf<uint8_t> pyramid;         // min/max pyramid over the leaf boxes (refit = 1: dxv_build and dxv_refit); cap: slots
    uint32_t T = 0;                  // triangles the scratch is in use for (0: none)
};

// A pair of events around one piece of a frame's work and the time last read from it.  armed: both events are in the frame's stream and
// nobody has read them yet -- the frame's next synchronisation does (timer_begin, timer_end, timer_read below).
struct Timer { hipEvent_t e0 = nullptr, e1 = nullptr; bool armed = false; float ms = 0; };
// ... and what a frame times.  The launch's pair and its queue build's are here for their events alone: when they are read is the launch's
// business (Frame::timed, lastRebuilt -> voxelize_ms, plan_ms), so they stand in front of kTimerFirstOperator: a synchronisation of the frame
// reads the armed pairs from there on (sync_launch), and a new operator's slot goes behind it.  The operators that run in batches of rounds
// form the tail from kTimerFirstBatched on: further batches move their second event, so their pairs are read where they are settled
// (settle_batched), and sync_launch stops in front of them.
enum TimerUse { kTimerLaunch, kTimerQueue, kTimerRender, kTimerDistance, kTimerMeshDistance, kTimerIso, kTimerOctree, kTimerComponents, kTimerMorph, kTimerMeasure, kTimerThickness,
                kTimerThickStage0, kTimerThickStageLast = kTimerThickStage0 + dxv::THICK_STAGES - 1,     // the six stages of a thickness, each a pair of its own
                kTimerPartition, kTimerPartStage0, kTimerPartStageLast = kTimerPartStage0 + dxv::PART_STAGES - 1,      // a partition and its six stages, likewise
                kTimerSkeleton, kTimerSight,
                kTimerFill, kTimerThin, kTimerGeodesic, kTimerAccess,
                kTimers,
                kTimerFirstOperator = kTimerRender, kTimerFirstBatched = kTimerFill };

struct dxv_ctx {
    int device = 0;
    hipStream_t ownStream = nullptr;
    hipStream_t stream = nullptr;
    hipStream_t copyStream = nullptr;    // dxv_update_vertices: the upload runs beside the frames' launches (made at its first call)
    bool vbCopyQueued = false;           // dxv_update_vertices_device left a copy into the vertex buffer on `stream` (until the next refit / build)
    std::string err;
    Options opt;                         // dxv_set_option (dxv_policy.h: the table of keys, what each accepts and means)

    // mesh (caller's layout; cap: bytes)
    DevBuf<float> vb;
    DevBuf<uint32_t> ib;
    uint32_t T = 0, V = 0;
    float bound[4] = {0, 0, 0, 0};
    bool haveMesh = false;

    // scene blob
    DevBuf<uint8_t> scene;
    size_t sceneBytes = 0;               // bytes of the scene (scene.cap: of the allocation behind it)
    SceneHeader hdr{};
    bool haveScene = false;
    bool haveHierarchy = false;      // dxv_build ran for the resident mesh: keys, links and parent words are in place for dxv_refit
                                     // (stays true when a refit fails on bad vertices: the next good update refits again)
    BuildScratch scratch;
    DevBuf<uint32_t> rootInfo;

    // outputs: FrameCount sets of grid / texel image / status words / redo list / stream, the way the reference's
    // Voxelizer owns FrameCount grids (Content/Voxelizer.h:24, :110); one scene and one set of lists serve them all
    struct Frame {
        hipStream_t ownStream = nullptr; // frames 1.. launch on a stream of their own; frame 0 on the context's stream
        DevBuf<uint8_t> grid;            // (cap: voxels; allocated in whole 256-byte lines)
        size_t gridBytes = 0;
        DevBuf<uint32_t> texels;         // (cap: voxels)
        DevBuf<uint32_t> status;         // [0] status bits, [1], [2] redo-list counters (alternating launches)
        DevBuf<uint64_t> redo;           // voxels whose LDS column was too small, finished by the redo pass
        uint32_t redoParity = 0;
        int lastRedoParity = -1;         // counter of the last launch (-1: that launch has none)
        Timer timers[kTimers];           // the frame's event pairs and the times read from them (TimerUse)
        int lastMode = 0;
        uint32_t lastZBlock = 1, lastZPeriod = 1;
        bool pending = false;            // a voxelize launch has not been checked by dxv_sync yet
        bool timed = true;               // ... and it was bracketed by the launch's two events (option events)
        bool lastCanFail = true;         // ... and it can report something (a walk's column can run out; the lists have no column)
        bool ready = false;              // status words, redo list, events and stream exist
        uint64_t gridVersion = 1;        // counts what rewrote the grid: launches and the edits in place (grid_rewritten).  What is made of the grid
                                         // remembers the version it was made of (Made, below) and is current exactly while the two are equal
        uint64_t clearSig = 0;           // the partial launch whose memset this grid still carries (launch_shape, traverse.hip); 0 = none
        bool ptrExposed = false;         // dxv_grid_device_ptr handed this grid out for writing: the caller may write through the pointer at any
                                         // time, so no memset is ever kept for it again (until the grid is reallocated)
        // launch fields of dxv_stats
        float voxelize_ms = 0.0f;
        uint32_t grid_dim = 0, z0 = 0, nz = 0, stack_entries = 0, redo_rays = 0, row_block = 0, list_entries = 0, list_res = 0;
        uint32_t plan_bricks = 0, plan_waves = 0;
        float plan_ms = 0.0f;
        // work queue of the lists kernel (plan_bricks.hip): the frame's own, written and read on the frame's stream only
        DevBuf<uint32_t> queue;          // two headers, then the slots (dxv_device.h); cap: 32-bit words
        uint32_t queueHdr = 0;           // the header (0 / 1) of the frame's current queue; the next build takes the other one ...
        bool queueOtherClear = false;    // ... which is all zero (cleared at the allocation, then by every build's k_plan_bricks)
        bool lastQueued = false;         // the frame's last launch went through the queue (dxv_sync reads its lengths for the stats)
        bool lastRebuilt = false;        // ... and built it (plan_ms is that build's)
        int lastPrepared = -1;           // the frame's last launch ran this PREPARED queue of the context (-1: none)
        uint32_t queueLens[16] = {};     // the lengths of the frame's eight queues and how many of each are heavy, as last read by dxv_sync ...
        uint64_t queueLenSig = 0;        // ... for the queue of this signature (clearSig); 0: not known
        hipEvent_t evEnd = nullptr;      // behind the frame's last launch, always recorded: what a refit on another stream waits for on the device
        bool usedLists = false;          // the frame's last launch went through the direction-space lists ...
        uint64_t listEpochUsed = 0;      // ... of this build (a build whose deferred check fails is withdrawn: settle_lists, sync_frame)
        // display pass (dxv_update_frame, dxv_render_async, dxv_render): what the frame renders with, its own so that frames render side by side
        RayCastCB cb{};                  // the ray-cast constants of the frame's last dxv_update_frame ...
        uint32_t cbWidth = 0, cbHeight = 0;   // ... and the viewport they were made for (0: none yet)
        DevBuf<uint8_t> empty;           // empty-brick flags of the frame's grid (empty_brick_bytes)
        uint32_t emptyDim = 0;           // grid side of the frame's last render with flags (0: none yet; dxv_debug_download reads them)
        // surface modes (surface.hip): the large triangles' lists of the frame's surface pass, its own (never the work queue's
        // buffers: a kept queue of the reference rule is still needed by the frame's next mode-0 launch)
        DevBuf<uint8_t> surf;
        // What is made of the grid, and what edits it in place: one record per operator (dxv_products.hip), each the frame's own so that frames
        // run theirs side by side.  A record's trim() releases what dxv_trim gives back -- the scratch of its making; what was made stays.
        // Made: whether the frame has had the product made, and of which grid version.  have goes with the buffer's content (false while a
        // product that is sized by the grid is being rebuilt: a failed allocation leaves "none yet"), version with the grid (0: being rebuilt).
        // How a caller reads a buffer of a product -- pointer, byte count, download -- is not the record's business: dxv_products.hip has a
        // descriptor per buffer (Readable) that names the record which guards it.  Flood, further down, is the part of a record that the two
        // flood operators share.
        struct Made {
            bool have = false;
            uint64_t version = 0;
            bool current(const Frame& f) const { return have && version == f.gridVersion; }
        };
        // distance field (distance.hip; dxv_distance_async): the field of the frame's grid and the scratch of its three passes
        struct Distance : Made {
            DevBuf<int32_t> field;           // (cap: voxels) 4 bytes per voxel, int32 or float32
            DevBuf<uint8_t> scratch;         // (cap: bytes) distance_scratch_bytes: the x pass's 16-bit values, the y pass's squares
            uint32_t dim = 0;                // grid side of the frame's last field
            int format = 0;                  // ... and its format (DXV_DIST_SQ_I32 / DXV_DIST_F32)
            void trim() { scratch.release(); }   // (the passes' scratch, 6 bytes per voxel; the field itself stays)
        } dist;
        // mesh distance field (mesh_distance.hip; dxv_mesh_distance_async): the field of the frame's last launch -- a slab's has nz slices --
        // and, when asked for, the nearest triangles; kept by dxv_trim
        struct MeshDistance : Made {
            DevBuf<float> field;             // (cap: voxels)
            DevBuf<uint32_t> tri;            // (cap: voxels)
            uint32_t dim = 0;                // grid side of the frame's last mesh distance field ...
            uint32_t nz = 0;                 // ... and its slices
            int format = 0;                  // ... its format
            bool hasTri = false;             // ... and whether the nearest triangles were made with it
            void trim() {}                   // (it has no scratch)
        } mdist;
        bool sceneReadPending = false;   // a mesh distance kernel that reads nodes and triangle records may still be running on the frame's stream: whatever
                                         // rewrites them on another stream (dxv_refit, ensure_nodes) waits for the frame's end event first; any
                                         // synchronisation of the frame clears it (the passes over the grid alone -- render, field, fill -- never set it)
        // exterior flood fill (fill.hip; dxv_fill_async): the two bit masks and the control block of the frame's fill
        struct Fill {
            DevBuf<uint8_t> scratch;         // (cap: bytes) fill_scratch_bytes
            bool pending = false;            // a batch is in the stream whose verdict (converged or not) nobody has read yet: the frame can still
                                             // report something, and its next synchronisation reads it and goes on if need be (settle_fill)
            int what = 0;                    // ... DXV_FILL_SOLID / DXV_FILL_INTERIOR, for the write-back of the batches that follow
            uint32_t batch = 0;              // ... rounds per batch (option fillrounds as it stood at dxv_fill_async)
            uint32_t rounds = 0;             // rounds of the frame's last fill so far, the confirming one included
                                             // (its timer's second event is recorded again behind every further batch, and settle_fill reads the pair)
            void trim() { scratch.release(); }   // (the masks, a quarter of a byte per voxel: sync_frames has settled every fill)
        } fill;
        // isosurface (isosurface.hip; dxv_isosurface_async): the triangle mesh of one of the frame's fields and the scratch of its extraction
        // (a bit per lattice cell, two counts per 64 cells, the scan's sums)
        struct Iso : Made {                  // (have: an empty mesh counts)
            DevBuf<uint8_t> vb;              // (cap: vertices) 24 bytes each
            DevBuf<uint32_t> ib;             // (cap: index words)
            DevBuf<uint8_t> scratch;         // (cap: bytes) iso_scratch_bytes
            uint32_t vertices = 0, triangles = 0;     // of the frame's last mesh
            void trim() { scratch.release(); }   // (the bits, counts and sums of an extraction; the mesh itself stays)
        } iso;
        // sparse voxel octree (octree.hip; dxv_octree_async): the nodes of the frame's grid and the scratch of their build (two bytes per cell of
        // levels 0 .. L - 1, a bit per cell, a count per 64 cells, the scan's sums)
        struct Octree : Made {
            DevBuf<uint32_t> nodes;          // (cap: nodes) 8 bytes each
            DevBuf<uint8_t> scratch;         // (cap: bytes) oct_scratch_bytes
            uint32_t levels = 0, count = 0;  // L and the nodes of the frame's last tree ...
            uint32_t levelFirst[12] = {};    // ... and the first node of every level, [L] the total
            bool expandPending = false;      // dxv_octree_expand_async read a CALLER's tree whose verdict (status word kOctStatusWord: an index that could not be
                                             // followed) nobody has read yet: the frame can still report something, and its next synchronisation reads it
            void trim() { scratch.release(); }   // (the dense cell words, bits and counts of a build; the nodes themselves stay)
        } oct;
        // connected components (components.hip; dxv_components_async): labels and table of the frame's grid and the scratch of their build
        // (two bits per voxel, a count per 64 voxels, the scan's sums; 32 bytes per component for the stats)
        struct Components : Made {
            DevBuf<uint32_t> labels;         // (cap: voxels)
            DevBuf<uint8_t> table;           // (cap: components) 24 bytes each
            DevBuf<uint8_t> scratch;         // (cap: bytes) comp_scratch_bytes
            DevBuf<uint8_t> work;            // (cap: bytes) the stats of a build, then the counters and keep flags of a select
            uint32_t count = 0, dim = 0;     // K and the grid side of the frame's last labelling ...
            int of = 0, connectivity = 0;    // ... and what it was asked for
            // the measures of that labelling (measure.hip; dxv_measure_async): K + 1 records of 96 bytes; stays with dxv_trim like the labels
            struct Measure : Made {          // (version: 0 once the frame is labelled again)
                DevBuf<uint8_t> table;       // (cap: records)
                uint32_t count = 0;          // K of the labelling the table was made of
            } measure;
            // the edit from the labels (dxv_components_select_async)
            struct Select {
                bool pending = false;        // its four counters are on their way into page-locked words: the frame's next synchronisation reads them
                int rule = 0;
                uint32_t components = 0;     // K of the labels that select edited from
                uint32_t kept = 0, dropped = 0;   // of the frame's last select, as of its last synchronisation
                uint64_t changed = 0;
            } select;
            void trim() { scratch.release(); work.release(); }   // (the masks, counts and stats of a labelling; labels and tables themselves stay)
        } comp;
        // morphology (morph.hip; dxv_morph_async): the bit masks and planes of the frame's morph
        struct Morph {
            DevBuf<uint8_t> scratch;         // (cap: bytes) morph_scratch_bytes
            bool pending = false;            // its two counters are on their way into page-locked words: the frame's next synchronisation reads them
            uint64_t set = 0, cleared = 0;   // of the frame's last morph, as of its last synchronisation
            void trim() { scratch.release(); }   // (the masks and planes: (R + 3) bits per voxel)
        } morph;
        // thinning (thin.hip; dxv_thin_async): the bit masks and the control block of the frame's thin
        struct Thin {
            DevBuf<uint8_t> scratch;         // (cap: bytes) thin_scratch_bytes
            bool pending = false;            // a batch is in the stream whose verdict (fixed point or not) nobody has read yet: the frame can still
                                             // report something, and its next synchronisation reads it and goes on if need be (settle_thin)
            int kind = 0;                    // ... DXV_THIN_CURVE / DXV_THIN_KERNEL, for the batches that follow
            uint32_t batch = 0;              // ... iterations per batch (option thinrounds as it stood at dxv_thin_async)
            uint32_t inBatch = 0;            // ... iterations of the batch in the stream (the last one of a bounded thin may be shorter)
            uint32_t left = 0;               // ... iterations max_iterations still allows behind that batch (bounded)
            bool bounded = false;            // ... max_iterations != 0
            uint32_t iterations = 0;         // iterations of the frame's last thin so far, the confirming one included
            uint64_t removed = 0;            // voxels it removed, as of the frame's last synchronisation
            bool converged = false;          // it stopped at an iteration that removed nothing (false: max_iterations stopped it first, or none yet)
            void trim() { scratch.release(); }   // (the masks, 3 1/8 bits per voxel: sync_frames has settled every thin)
        } thin;
        // local thickness (thickness.hip; dxv_thickness_async): the map and the histogram of the frame's grid and the scratch of their making (two
        // fields, a byte per voxel, the fields' passes)
        struct Thickness : Made {
            DevBuf<uint32_t> map;            // (cap: voxels)
            DevBuf<unsigned long long> hist; // (cap: bins)
            DevBuf<uint8_t> scratch;         // (cap: bytes) thickness_scratch_bytes
            uint32_t dim = 0, cap = 0;       // grid side and cap_sq of the frame's last map
            bool pending = false;            // its four counters are on their way into page-locked words: the frame's next synchronisation reads them
            uint64_t centres = 0, items = 0, tested = 0, sent = 0;   // of the frame's last thickness, as of its last synchronisation
            void trim() { scratch.release(); }   // (the fields, bytes and passes, 15 bytes per voxel; map and histogram themselves stay)
        } thick;
        // maximal-ball partition (partition.hip; dxv_partition_async): labels, table and throats of the frame's grid, the scratch of their making
        // (field or parents, keys, roots, the mips, the passes) and the work sized by its counts (the regions' stats, the sort of the faces)
        struct Partition : Made {
            DevBuf<uint32_t> labels;         // (cap: voxels)
            DevBuf<uint8_t> table;           // (cap: regions) 32 bytes each
            DevBuf<uint32_t> throats;        // (cap: throats) 20 bytes each
            DevBuf<uint8_t> scratch;         // (cap: bytes) partition_scratch_bytes
            DevBuf<uint8_t> work;            // (cap: bytes) partition_work_bytes
            uint32_t dim = 0, cap = 0;       // grid side and cap_sq of the frame's last partition ...
            int of = 0;                      // ... what it was asked for ...
            bool hasThroats = false;         // ... and whether the throats were made with it
            uint32_t regions = 0, throatCount = 0;
            uint64_t faces = 0;              // its interface faces (0 without throats)
            bool pending = false;            // its two counters are on their way into page-locked words: the frame's next synchronisation reads them
            uint64_t cellsTested = 0, voxelsTested = 0;   // of the frame's last partition, as of its last synchronisation (option partstages)
            void trim() { scratch.release(); work.release(); }   // (22 bytes per voxel and the sort's buffers; labels, table and throats themselves stay)
        } part;
        // Flood: what the two operators that flood the members from seeds in batches of rounds keep alike (geodesic and access, below; their
        // host side shares its seed handling, its accounting and its work-info getter: dxv_products.hip)
        struct Flood : Made {
            DevBuf<uint32_t> seeds;          // (cap: indices) the seeds of a list
            std::vector<uint32_t> list;      // the caller's list, copied before the operator's _async returns: what the upload reads
            bool pending = false;            // a batch is in the stream whose verdict (fixed point or not) nobody has read yet: the frame's next
                                             // synchronisation reads it and goes on if need be (settle_geodesic, settle_access)
            uint32_t batch = 0;              // ... rounds per batch (option georounds / accessrounds as it stood at the operator's _async)
            uint32_t rounds = 0;             // rounds of the frame's last flood so far, the confirming one included
            uint64_t tilesRun = 0;           // ... the tiles its rounds ran, the most of one round, and the rounds with fewer than kGeoSparseTiles
            uint32_t mostLive = 0, sparseRounds = 0;
            uint64_t seedsUsed = 0, reached = 0, unreached = 0;     // its tally, as of the frame's last synchronisation
        };
        // geodesic distance (geodesic.hip; dxv_geodesic_async): the map of the frame's grid, and the scratch of its making -- control block, live
        // flags, queue; the seeds of a list; the words of a path
        struct Geodesic : Flood {
            DevBuf<uint32_t> map;            // (cap: voxels)
            DevBuf<uint8_t> scratch;         // (cap: bytes) geodesic_scratch_bytes
            DevBuf<uint32_t> path;           // (cap: words) dxv_geodesic_path: length, status, voxel indices
            uint32_t dim = 0;                // grid side of the frame's last map
            int metric = 0;                  // ... DXV_GEO_FACES / DXV_GEO_CHAMFER, for the batches that follow and for the path
            uint32_t limit = 0;              // ... its limit (0: none)
            uint32_t farthest = 0, farthestVoxel = 0xFFFFFFFFu;     // the rest of its tally
            void trim() { scratch.release(); seeds.release(); path.release(); }   // (control block, flags and queue, 6 bytes per 8^3 tile, a list's seeds, a path's words; the map itself stays)
        } geo;
        // access radius and intrusion map (access.hip; dxv_access_async): the two maps of the frame's grid and their histograms, and the scratch of
        // their making -- control block, live flags, queue, the radius field and its passes, with the intrusion map a thickness's scratch; the
        // seeds of a list.  Behind its last batch the frame's synchronisation also enqueues paint and histograms (settle_access).
        struct Access : Flood {
            DevBuf<uint32_t> map;            // (cap: voxels) A
            DevBuf<uint32_t> intrusion;      // (cap: voxels) I, when asked for
            DevBuf<unsigned long long> hist, histI;      // (cap: bins)
            DevBuf<uint8_t> scratch;         // (cap: bytes) access_scratch_bytes
            uint32_t dim = 0, cap = 0;       // grid side and cap_sq of the frame's last maps
            int of = 0, connectivity = 0;    // ... what they were asked for, for the batches that follow
            bool wantIntrusion = false;      // ... and whether the intrusion map is made with them
            uint32_t cull = 0;               // ... option thickcull as it stood at dxv_access_async, for the paint
            uint32_t widest = 0, widestVoxel = 0xFFFFFFFFu;         // the rest of its tally
            void trim() { scratch.release(); seeds.release(); }     // (control block, flags, queue, fields and passes; the maps and histograms themselves stay)
        } acc;
        // skeleton graph (skeleton.hip; dxv_skeleton_async): labels and the two tables of the frame's grid, the scratch of their making (four bits
        // per voxel of masks, the root bits, the counts, the scan's sums) and the work sized by K and B (the nodes' stats, then a prune's flags)
        struct Skeleton : Made {
            DevBuf<uint32_t> labels;         // (cap: voxels)
            DevBuf<uint8_t> nodes;           // (cap: nodes) 32 bytes each
            DevBuf<uint8_t> branches;        // (cap: branches) 48 bytes each
            DevBuf<uint8_t> scratch;         // (cap: bytes) skel_scratch_bytes
            DevBuf<uint8_t> work;            // (cap: bytes) the nodes' stats of a build, then the counters and flags of a prune
            uint32_t dim = 0;                // grid side of the frame's last skeleton
            uint32_t nodeCount = 0, branchCount = 0;
            uint64_t endVoxels = 0, curveVoxels = 0, junctionVoxels = 0;
            // the edit from the tables (dxv_skeleton_prune_async)
            struct Prune {
                bool pending = false;        // its two counters are on their way into page-locked words: the frame's next synchronisation reads them
                uint32_t branches = 0;       // of the frame's last prune, as of its last synchronisation
                uint64_t voxels = 0;
            } prune;
            void trim() { scratch.release(); work.release(); }   // (the masks, bits, counts and stats; labels and tables themselves stay)
        } skel;
        // line-of-sight map (sight.hip; dxv_sight_async): the map of the frame's grid and its tally, and the scratch of their making -- the member
        // mask and a bit plane per requested direction
        struct Sight : Made {
            DevBuf<uint32_t> map;            // (cap: voxels)
            DevBuf<uint8_t> scratch;         // (cap: bytes) sight_scratch_bytes
            uint32_t dim = 0;                // grid side of the frame's last map
            int of = 0;                      // ... what it was asked for
            uint32_t directions = 0;         // ... and the directions it was made with
            bool pending = false;            // its tally is on its way into page-locked words: the frame's next synchronisation reads it
            unsigned long long tally[68] = {};   // of the frame's last map, as of its last synchronisation (dxv_sight.h: SightTally)
            void trim() { scratch.release(); }   // (the mask and the planes, up to 27 bits per voxel; the map itself stays)
        } sight;
        // What a synchronisation of the frame and a launch need to know of all that, without naming an operator.
        // grid_unsettled: the grid may not be final yet -- a fill or a thin whose verdict is not in, an expansion from a caller's tree that can
        // still report; unsettled: ... or a geodesic or an access, which only read the grid, has further batches to go in front of whatever comes next.
        bool grid_unsettled() const { return fill.pending || thin.pending || oct.expandPending; }
        bool unsettled() const { return grid_unsettled() || geo.pending || acc.pending; }
        // a launch replaces the grid: a fill of it that has not converged yet is dropped (its batch in the stream ends in front of the launch), a
        // thin likewise (it stopped where that batch ended), and a geodesic map of it (stale from here on, nobody can read it)
        void drop_unsettled()
        {
            fill.pending = false;
            if (thin.pending) { thin.pending = false; thin.converged = false; }
            geo.pending = false;
            acc.pending = false;
        }
        void trim_products() { dist.trim(); mdist.trim(); fill.trim(); iso.trim(); oct.trim(); comp.trim(); morph.trim(); thin.trim(); thick.trim(); part.trim(); geo.trim(); acc.trim(); skel.trim(); sight.trim(); }
    };
    Frame frames[DXV_FRAME_COUNT];
    uint32_t cur = 0;                    // dxv_set_frame
    bool texels = false;
    DevBuf<unsigned long long> count;
    DevBuf<uint8_t> packed;              // (cap: bytes of the packed grid)
    DevBuf<uint32_t> image;              // (cap: pixels)
    Lists lists;
    uint32_t listResFloor = 0;       // automatic resolution: not below this (512 once a scene of 20 k triangles or more that was not refitted
    bool listFloorTried = false;     // is launched AGAIN: a static scene -- the finer map is 10 - 20 % faster at every grid size since texels
                                     // outside a triangle's outline get no entry, and costs a build of 1.5 - 2 x)
    bool refitted = false;           // dxv_refit has run since dxv_build: the mesh is being animated, its lists are built for one launch
    DevBuf<uint8_t> listScratchA, listScratchB;   // scratch of the list build, kept between builds (a refit rebuilds them); cap: bytes
    // The dynamic case (a mesh refitted every frame, XUSGRayTracing.h:13-22) with ONE host round trip per frame instead of four:
    //  * dxv_refit queues the lists' counting pass behind its own kernels when the scene had lists (specRes: the map it counted
    //    on) and reads root box and entry total in one synchronisation;
    //  * a build made inside a launch does not wait for its own end: the launch is queued behind it, and the one thing the host
    //    must still look at -- a texel with more entries than its 16-bit count holds -- is looked at when the frame is
    //    synchronised (settle_lists); lists that fail there are withdrawn and the frame is launched again through the tree.
    // Everything the device reports goes through page-locked words (a copy into pageable memory blocks the host until the
    // stream has drained: 30 us of idle GPU per copy in the refit loop's trace).
    struct Pinned {
        uint32_t rootInfo[16];
        unsigned long long listTotal;
        uint32_t listLongest, pad;
        uint32_t listStarts[2];                          // non-empty texels, texels of more than 8 entries (dirmap_starts): start_table_pays
        uint32_t preparedLens[16 * 64];                  // the sixteen count words of a queue that is being prepared (as PerFrame::queueLens)
        struct PerFrame {
            uint32_t status[4];
            uint32_t queueLens[16 * 64];                 // the sixteen count words of the frame's queue (light and heavy bricks of the eight queues; each in a 256-byte line of its own)
            uint32_t fillCtl[64];                        // the control block of the frame's last fill batch (kFillMaxRounds words)
            unsigned long long isoTotals[2];             // vertices and quads of the mesh the frame is extracting: sizes its buffers
            unsigned long long octTotals[12];            // level_first[0 .. L] of the tree the frame is building: sizes its node buffer
            unsigned long long compTotal;                // K of the labelling the frame is building: sizes its table
            unsigned long long compSel[4];               // kept, dropped, voxels changed and the largest component's key of the frame's last select
            unsigned long long morphCount[2];            // voxels set and voxels cleared by the frame's last morph
            dxv::ThinControl thinCtl;                    // the control block of the frame's last thin batch and the voxels removed so far
            unsigned long long thickCount[4];            // centres painted, work items, voxels tested and atomics sent of the frame's last thickness
            unsigned long long partTotals[2];            // K and the interface faces of the partition the frame is making: size its table and its sort
            unsigned long long partPairs[2];             // T of that partition: sizes its throats
            unsigned long long partCount[2];             // mip cells and voxels tested by the search of the frame's last partition
            dxv::GeoControl geoCtl;                      // the control block of the frame's last geodesic batch and the tally behind it
            dxv::GeoControl accCtl;                      // ... of the frame's last access batch, likewise
            unsigned long long skelTotals[5];            // K, B and the end, curve and junction voxels of the skeleton the frame is making: K and B size its tables
            unsigned long long sightTally[68];           // the tally of the frame's last line-of-sight map
            unsigned long long skelPrune[2];             // branches and voxels removed by the frame's last prune
        } frame[DXV_FRAME_COUNT];
    };
    Pinned* pin = nullptr;
    hipEvent_t evList[4] = {};       // around the counting pass, around the rest of the build
    uint32_t specRes = 0;            // the counting pass for the current scene has run on this map (records, counts, total in place)
    bool listCheckPending = false;   // lists in use whose longest texel has not been looked at yet
    hipStream_t listCheckStream = nullptr;
    uint64_t withdrawnEpoch = 0;     // listEpoch of the last build that failed its deferred check
    uint32_t launchesOfScene = 0;    // reference-rule launches since the scene last changed (build / refit / import)
    uint64_t listEpoch = 0;          // counts list builds / imports: a frame's queue belongs to the lists it was probed against
    uint64_t sceneEpoch = 0;         // counts builds / refits / imports
    FarMap farMap;
    uint64_t boxLaunchEpoch = 0;     // the scene epoch boxLaunchesOfScene counts for
    uint32_t boxLaunchesOfScene = 0; // reference-rule launches over the brick box (tree walks, plan = 0) since the scene last changed
    ListsOccupancy occupancy;        // what the runtime said about the brick kernels on this context's device, asked at first use
    // PREPARED work queues (dxv_prepare_launch; the host mirrors' Init with a grid hint): the queue of a (lists, grid, partition) is a pure
    // function of them, like the lists are of the scene -- built once when they are fixed, kept with the context (not with a frame:
    // every frame's launches read it), dropped by whatever changes the scene or its lists.  A launch of a prepared partition clears
    // its grid and has the hardware deal out the queued bricks; any other launch builds its queue itself (plan = 2).
    struct Prepared {
        uint64_t epoch = 0;              // listEpoch of the lists it was probed against (0: the slot is free)
        uint32_t N = 0, z0 = 0, nz = 0, zBlock = 0, zPeriod = 0, regionBits = 0, planHeavy = 0;
        DevBuf<uint32_t> mem;            // header (the build's counters), then 8 x cap brick words; cap: words
        uint32_t cap = 0;
        DevBuf<uint32_t> live;           // one bit per brick of the partition: queued or not (what the launch's clear reads); cap: words
        uint32_t lens[16] = {};          // the eight lengths and how many of each are heavy
        uint32_t bricks = 0;
        float ms = 0.0f;                 // its build on the device
        uint64_t used = 0;               // (the least recently used slot goes when all are taken)
    };
    static constexpr uint32_t kPreparedSlots = 16;   // (eight shares of a looped 8-rank partition and a few whole grids)
    Prepared prepared[kPreparedSlots];
    uint64_t preparedClock = 0;
    float prepareMs = 0.0f;          // device time of the last dxv_prepare_launch* (0: it found the partition prepared)
    RowLists rowLists;
    uint32_t parityLaunchesOfScene = 0;
    int nodesStale = 0;              // what a build / refit left behind (ensure_nodes brings it up to date before anything reads it):
                                     // 1 = the four-box copy (nodes64); 2 = every node box (dxv_refit stopped at the pyramid: deferBoxes)

    hipEvent_t ev[10] = {};
    dxv_stats stats{};
    int stackNow = 20;       // adaptive: LDS stack entries per thread currently in use for this scene
};

namespace dxvhost {

int fail(dxv_ctx* c, const char* fmt, ...);          // dxv_api.hip: message into the context (or the create error), returns 1

#define DXV_HIP(c, call)                                                                          \
    do {                                                                                          \
        hipError_t e_ = (call);                                                                   \
        if (e_ != hipSuccess) return fail((c), "%s failed: %s", #call, hipGetErrorString(e_));    \
    } while (0)

using Frame = dxv_ctx::Frame;
inline Frame& cur_frame(dxv_ctx* c) { return c->frames[c->cur]; }
inline const Frame& cur_frame(const dxv_ctx* c) { return c->frames[c->cur]; }
inline hipStream_t frame_stream(dxv_ctx* c, uint32_t i) { return i == 0 ? c->stream : c->frames[i].ownStream; }
inline hipStream_t cur_stream(dxv_ctx* c) { return frame_stream(c, c->cur); }
inline Node* scene_nodes(dxv_ctx* c) { return reinterpret_cast<Node*>(c->scene.p + c->hdr.offNodes); }
inline Node32* scene_nodes32(dxv_ctx* c) { return reinterpret_cast<Node32*>(c->scene.p + c->hdr.offNodes32); }
inline Node64* scene_nodes64(dxv_ctx* c) { return reinterpret_cast<Node64*>(c->scene.p + c->hdr.offNodes64); }
inline TriPos* scene_tripos(dxv_ctx* c) { return reinterpret_cast<TriPos*>(c->scene.p + c->hdr.offTriPos); }
inline TriNrm* scene_trinrm(dxv_ctx* c) { return reinterpret_cast<TriNrm*>(c->scene.p + c->hdr.offTriNrm); }
// what a kernel's parameters say about the scene: hierarchy, triangle records, root box ...
inline void scene_params(dxv_ctx* c, SceneView& sc)
{
    sc.nodes = scene_nodes32(c); sc.wide = c->hdr.hasWide ? scene_nodes64(c) : nullptr; sc.triPos = scene_tripos(c); sc.triNrm = scene_trinrm(c);
    memcpy(sc.rootLo, c->hdr.rootLo, 12);
    memcpy(sc.rootHi, c->hdr.rootHi, 12);
}
// ... and about its direction-space lists
inline void lists_params(const dxv_ctx* c, SceneView& sc)
{
    sc.dmCells = c->lists.cells.p; sc.dmEntries = c->lists.entries.p; sc.dmR = c->lists.res;
    sc.dmStarts = start_table_used(c->opt.starttable, c->lists.startsPay) ? c->lists.starts.p : nullptr;
    sc.dmStartCells = sc.dmStarts ? c->lists.startCells.p : nullptr;
}
inline uint32_t z_shift(uint32_t zBlock)
{
    uint32_t shift = 0;
    while ((1u << shift) < zBlock) ++shift;
    return shift;
}
// the column an adaptive launch of this scene starts with: option stack0, or less when the tree is lower
inline int initial_stack(const dxv_ctx* c)
{
    return stack_round_up((int)(c->hdr.treeHeight + 3 < (uint32_t)c->opt.stack0 ? c->hdr.treeHeight + 3 : (uint32_t)c->opt.stack0));
}
// the ray rule a launch of this mode runs (mode 3 is the reference rule's launch, then the surface pass; mode 2 runs none)
inline int ray_rule(int mode) { return mode == DXV_MODE_REFERENCE_SURFACE ? DXV_MODE_REFERENCE : mode; }
inline float elapsed(hipEvent_t a, hipEvent_t b)
{
    float ms = 0.0f;
    if (hipEventElapsedTime(&ms, a, b) != hipSuccess) return -1.0f;
    return ms;
}

// The grid of a frame was rewritten, by a launch or in place: whatever was made of it before -- fields, the mesh, the tree, labels, maps -- is
// stale from here on.
inline void grid_rewritten(Frame& f) { ++f.gridVersion; }
// ... in place: the grid also stops being what the frame's last launch wrote, so a kept queue's zeros are gone (the next launch clears
// everything; the caller holds no pointer because of this, so ptrExposed stays).  A launch keeps its own account of that.
inline void edited_in_place(Frame& f) { f.clearSig = 0; grid_rewritten(f); }
// A frame's timers.  begin: the pair is disarmed before its first event is recorded again -- a first event recorded again and an old second
// one are no pair; end: armed once the second event is in the stream (whatever the caller enqueues behind it: both events can be read); read: what a synchronisation of the frame does with an armed pair.
inline hipError_t timer_begin(Timer& t, bool timed, hipStream_t s)
{
    t.armed = false;
    return timed ? hipEventRecord(t.e0, s) : hipSuccess;
}
inline hipError_t timer_end(Timer& t, bool timed, hipStream_t s)
{
    const hipError_t e = timed ? hipEventRecord(t.e1, s) : hipSuccess;
    t.armed = timed && e == hipSuccess;
    return e;
}
inline void timer_read(Timer& t)
{
    if (t.armed) { t.ms = elapsed(t.e0, t.e1); t.armed = false; }
}

// dxv_api.hip
void layout_scene(SceneHeader& h, uint32_t T, uint32_t V, bool wide);
int alloc_scene(dxv_ctx* c, uint32_t T, uint32_t V, bool wide);
int alloc_scratch(dxv_ctx* c, uint32_t T);
void fill_build_buffers(dxv_ctx* c, BuildBuffers& b);
int wait_scene_readers(dxv_ctx* c, hipStream_t stream);   // `stream` waits, on the device, for the frames' passes that still read the scene (sceneReadPending)
int ensure_nodes(dxv_ctx* c, hipStream_t stream);       // the hierarchy's traversal copies after a refit that skipped them
enum class SceneCause { mesh, build, refit, import };
void scene_changed(dxv_ctx* c, SceneCause why);         // everything a new mesh, a build, a refit or an import invalidates
void fill_scene_stats(dxv_ctx* c);                      // the scene's fields of dxv_stats, from the header
// dxv_frames.hip
int ensure_far_map(dxv_ctx* c, hipStream_t s);             // the far-radius map of a scene without lists (dirmap_far), current for the scene when this returns 0
void drop_prepared(dxv_ctx* c);                            // whatever changes the scene or its lists calls this (the slots keep their memory)
int frame_prepare(dxv_ctx* c, uint32_t i);
int sync_frame(dxv_ctx* c, uint32_t i);
int sync_frames(dxv_ctx* c);
bool use_wide(const dxv_ctx* c, int mode);
int safe_stack(const dxv_ctx* c, int mode);
int launch_now(dxv_ctx* c, uint32_t frame, bool relaunch = false);
int render_frame(dxv_ctx* c, const RayCastCB& cb, uint32_t width, uint32_t height, uint8_t* dst, size_t pitch, bool timed);
bool frame_renderable(const Frame& f);
int settle_frame_launch(dxv_ctx* c);                       // the host waits for the selected frame only when it can still report something
// `ptr` is device memory of this context's device and `need` bytes from it lie inside its allocation: 0; 1 with the message set; or, where
// the range does not fit, 2 with the bytes the allocation has from `ptr` on in *room -- the sentence about that is the caller's own
int check_device_range(dxv_ctx* c, const char* who, const void* ptr, size_t need, size_t* room);
// argument checks of the entries that take a grid, a slab of it or a rank's interleaved share: 0, or 1 with the message set
int check_grid(dxv_ctx* c, const char* who, uint32_t N, bool orZero = false);
int check_slab(dxv_ctx* c, const char* who, uint32_t N, uint32_t z0, uint32_t nz);
int check_interleave(dxv_ctx* c, const char* who, uint32_t N, uint32_t rank, uint32_t world, uint32_t zblock);
// dxv_products.hip
void read_products(dxv_ctx* c, uint32_t i);                // the counters of the frame's last select, morph and thickness, once its stream has been waited for
int settle_fill(dxv_ctx* c, uint32_t i);                   // the verdict of the frame's last fill batch; further batches until one has converged (settle_batched)
int settle_thin(dxv_ctx* c, uint32_t i);                   // ... of the frame's last thin batch; further batches until the fixed point or max_iterations
int settle_access(dxv_ctx* c, uint32_t i);                 // ... of the frame's last access batch; further batches, then the intrusion map and the histograms
int settle_geodesic(dxv_ctx* c, uint32_t i);               // ... of the frame's last geodesic batch; further batches until a round finds nothing live
int settle_expand(dxv_ctx* c, uint32_t i);                 // the verdict of an expansion from a caller's tree
// dxv_lists.hip
struct ListScratchA { DirRecord* rec; uint32_t *counts, *offsets, *pairs, *sums; unsigned long long* total; size_t bytes; };
ListScratchA list_scratch_a(uint8_t* base, uint32_t T);
uint32_t list_resolution(const dxv_ctx* c);
int settle_lists(dxv_ctx* c);
int build_lists(dxv_ctx* c, hipStream_t stream, uint64_t firstLaunchVoxels = 0, bool defer = false);
int build_plists(dxv_ctx* c, hipStream_t stream);

} // namespace dxvhost
