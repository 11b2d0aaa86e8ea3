// dxv_device.h -- declarations shared by the HIP translation units of libdxv.so.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "dxv_types.h"
#include "dxv_trace.h"
#include "dxv_scratch.h"

namespace dxv {

// The grid operators (distance.hip .. partition.hip below) describe their scratch memory ONCE, in the carve function beside their params in
// their rule header (dxv_scratch.h has the Carve; dxv_distance.h, dxv_fill.h, ... the functions): X_scratch_bytes is that function over a null
// base, the layout the same function over the allocation.  Here stand the launches alone.

// radix_sort.hip
// plan: the diagnostic override (option sortbits) as ONE caller snapshot of radix_sort_plan(), -1: read it now
hipError_t radix_sort_keys_bits(uint64_t* keys, uint64_t* tmp, uint32_t n, uint32_t* hist, int loBit, int numBits, uint64_t** result,
                                hipStream_t s, int plan = -1);
int radix_sort_passes(uint32_t n, int numBits, int plan = -1);     // how many times that sort swaps keys and tmp
int radix_sort_plan();                              // the process-wide override as it stands (a build asks once)
void radix_sort_set_plan(int v);                    // diagnostic (option sortbits)

// lbvh.hip -- device-side build of the scene blob.
struct BuildBuffers {
    const float* vb;        // V x 6
    const uint32_t* ib;     // 3T
    uint32_t T, V;
    float bound[4];
    uint64_t* keys;         // T
    uint64_t* keysTmp;      // T
    uint32_t* hist;         // radix_sort_hist_words(T)
    uint32_t* parents;      // (T-1) internal + T leaf words: (parent << 1) | side
    uint32_t* flags;        // T-1 arrival counters (atomic refit) / ready flags (sweep refit)
    uint32_t* flags2;       // T-1: far end of every node's run of leaves (k_hierarchy -> pyramid refit)
    void* pyramid;          // pyramid_slots(T) x 28 B: min/max pyramid over the leaf boxes + deepest leaf, or NULL (sweeps)
    uint32_t* rootInfo;     // 8 words: rootLo[3], rootHi[3] (float bits), height, done
    Node* nodes;            // max(T-1,1), exact boxes
    Node32* nodes32;        // max(T-1,1), traversal copy
    Node64* nodes64;        // max(T-1,1), wide traversal copy
    TriPos* triPos;         // T
    TriNrm* triNrm;         // T
    bool deferCopies;       // leave the four-box copy (nodes64) stale: lbvh_traversal_copies brings it up to date when a walk needs it (nodes32 always is)
    bool deferBoxes;        // lbvh_refit only (pyramid refit): stop after the min/max pyramid -- root box from its top, node boxes left stale
                            // until lbvh_refit_boxes; the lists are built from the triangle records alone
};
struct BuildTimes { float prep, sort, hierarchy, refit; };
// refitMode: 0 = one pass, bottom-up with per-node arrival counters; 1 = level-synchronous sweeps
hipError_t lbvh_build(const BuildBuffers& b, int refitMode, hipStream_t s, hipEvent_t ev[5]);
uint32_t pyramid_slots(uint32_t T);
hipError_t lbvh_refit(const BuildBuffers& b, int refitMode, uint32_t treeHeight, hipStream_t s, hipEvent_t ev[2]);
hipError_t lbvh_traversal_copies(const BuildBuffers& b, hipStream_t s);   // nodes32 -> nodes64: the four-box copy the wide tree walks read
hipError_t lbvh_refit_boxes(const BuildBuffers& b, hipStream_t s);        // what a refit with deferBoxes left undone: node boxes from the pyramid it made, then the copies

// dirmap.hip -- direction-space lists of the reference rule (dxv_dirmap.h)
struct DirEntry;
struct DirRecord;
struct DirCell;
hipError_t dirmap_count(const TriPos* triPos, uint32_t T, uint32_t R, DirRecord* rec, uint32_t* counts, uint32_t* pairs, uint32_t* wideList, unsigned long long* total, bool lateral, hipStream_t s, uint32_t stride = 1);   // lateral: option lateralpad (dxv_dirmap.h: dm_lateral_pad)
hipError_t dirmap_fill(uint32_t T, uint32_t R, const DirRecord* rec, const uint32_t* counts, const uint32_t* pairs, const unsigned long long* total,
                       uint32_t* offsets, uint32_t* sums, uint64_t* keys, uint64_t* keysTmp, uint32_t* hist, uint32_t n, DirCell* cells, DirEntry* entries, uint32_t* longest,
                       hipStream_t s);

// max-mips of the texels' far radii and entry counts (dxv_dirmap.h: dm_mip_max), dm_mip_buffer_words(R) 16-bit words: what the launch's work queue is probed against
hipError_t dirmap_mip(const DirCell* cells, uint32_t R, uint16_t* mip, hipStream_t s);
hipError_t dirmap_starts(const DirCell* cells, uint32_t R, const DirEntry* entries, uint32_t* starts, DirCell* startCells, hipStream_t s);   // starts: 6 R R words (dm_start_word) + two counters: non-empty texels, texels of more than 8 entries; startCells: 6 R R cells (dm_start_cell)

// the far-radius map of a scene WITHOUT lists (a tree walk's brick test): far32 = 6 R R words of scratch, cells = 6 R R, mip = dm_mip_buffer_words(R)
hipError_t dirmap_far(const TriPos* triPos, uint32_t T, uint32_t R, uint32_t* far32, DirCell* cells, uint16_t* mip, hipStream_t s);

// consistency of a list section that arrived in a blob (dxv_scene_import): out[0] = cells whose range leaves the entries,
// out[1] = entries whose triangle slot is >= T
hipError_t dirmap_validate(const DirCell* cells, uint32_t R, const DirEntry* entries, uint32_t n, uint32_t T, uint32_t* out, hipStream_t s);

// offsets[0 .. n) = exclusive scan of counts[0 .. n); sums: ceil(n / 1024) words of scratch
hipError_t scan_exclusive(const uint32_t* counts, uint32_t n, uint32_t* sums, uint32_t* offsets, hipStream_t s);

// parity_lists.hip -- row lists of the parity rule (pl_rect, dxv_dirmap.h); validate: as dirmap_validate
hipError_t parity_lists_validate(const uint32_t* cells, uint32_t R, const uint32_t* entries, uint32_t n, uint32_t T, uint32_t* out, hipStream_t s);
hipError_t parity_lists_total(const TriPos* triPos, uint32_t T, uint32_t R, unsigned long long* total, hipStream_t s);
hipError_t parity_lists_fill(const TriPos* triPos, uint32_t T, uint32_t R, uint32_t* counts, uint32_t* offsets, uint32_t* sums, uint32_t* cells,
                             uint32_t* entries, hipStream_t s);

// traverse.hip / plan_bricks.hip / voxelize_lists.hip / parity_rows.hip -- one launch of a ray rule over a partition
struct VoxelizeParams {
    SceneView scene;
    uint8_t* grid;          // N*N*nz bytes
    uint32_t* texels;       // optional N*N*nz words
    uint32_t* status;       // status[0] bit 0: a ray could not be finished (redo list full, or the redo pass itself ran out)
                            // status[1 + parity], status[2 - parity]: rays on the redo list of this / the next launch
    uint64_t* redo;         // voxel ids (local index into grid) whose LDS column was too small: finished by k_voxelize_redo
    uint32_t redoCap;       // entries of `redo`
    uint32_t redoParity;    // which of the two counters this launch appends to
    uint32_t N, z0, nz;     // nz = slices written by this launch (local index lz in [0, nz))
    uint32_t zBlock, zPeriod; // global slice of lz: z0 + (lz / zBlock) * zPeriod + lz % zBlock
    uint32_t zShift;          // log2(zBlock) when the partition is block-cyclic (zBlock is a power of two)
    uint32_t superX, superY;  // brick super-blocks per axis (filled by the launcher)
    uint32_t nbx, nby, nbz;   // bricks launched per axis and their offset: only the part of the grid
    uint32_t bx0, by0, bz0;   //   that the root early-out cannot clear (the rest is memset to 0)
    int mode;
    uint32_t morton;        // 1: Morton brick order (default), 0: linear x,y,z order
    uint32_t mortonBits;    // filled by the launcher
    uint32_t regionBits;    // log2 of the bricks per XCD region
    uint32_t queued;        // 1: postponed-leaf traversal (default), 0: leaves tested on the spot
    uint32_t subbox;        // 1: launch only bricks the root early-out cannot clear (default)
    uint32_t wide;          // 1: reference rule walks the wide nodes (default when the stack bound allows)
    uint32_t lists;         // 1: reference rule reads the direction-space lists of p.scene (no tree walk)
    uint64_t* clearSig;     // host word of the frame (or NULL): signature of the partial launch whose memset the grid still carries -- the same launch again skips the memset
    uint32_t ablate;        // timing-only builds of the lists kernel (wrong grids; tools/ablate.py), 0 = the real kernel
    uint32_t* queue;        // work queue of the lists kernel (plan_bricks.hip): the header this launch uses (64 heads, 8 lengths, every word in a line of its own)
    uint32_t* queueSlots;   // ... its 8 x queueCap brick words
    uint32_t* queueZero;    // ... the frame's OTHER header, cleared by k_plan_bricks for the launch that builds the next queue (or NULL)
    uint32_t queueCap;
    uint32_t planRegionBits; // log2 of the run of consecutive Morton bricks that goes to one queue (6, 7 or 8)
    uint32_t planHeavy;     // a brick that can look into a list of more entries than this goes to the front of its queue; 0: the scene's own "long list" (k_dm_heavy_thresholds)
    uint32_t planClear;     // 1: k_plan_bricks also clears the grid (and the texel image): no memset in front of it
    uint32_t queueWaves;    // persistent waves to launch; 0 = queueSevenths / 7 of what the device holds at once
    uint32_t queueSevenths; // (dxv_policy.h: queue_waves_sevenths; 0 = 7)
    uint32_t queueHeads;    // heads per queue the persistent waves draw from: 1, 2, 4 or 8
    uint32_t queueMinBricks; // persistent waves beyond one per this many bricks of an XCD's share leave at once (0: all stay)
    const uint16_t* mip;    // max-mip of the lists' far radii (dxv_dirmap.h), what k_plan_bricks probes the bricks against
    uint32_t mipR;          // brick-box launches (k_voxelize, 4^3 bricks, reference rule): the map `mip` was made on -- every workgroup makes
                            // the queue's brick test itself and a brick that cannot hold a live ray is zeroed and left; 0: no test
    uint32_t listedWaves;   // k_voxelize_listed without the texel image fits eight waves per SIMD (64 VGPRs, 32 workgroups per CU): 8 .. 32 = held at so many
                            // workgroups per CU by LDS it does not use; 0: by grid and map (listed_lds_pad, voxelize_lists.hip; option listedwaves)
    uint32_t* liveMask;     // k_plan_bricks: one bit per brick of the partition, id (bz nbx + by) nbx + bx, set for every queued brick (or NULL):
                            // what the clear of a launch through a PREPARED queue reads (only the bricks nobody runs are zeroed)
};
// traverse.hip -- tree walks (and the lists, plan = 0) over the brick box
hipError_t launch_voxelize(const VoxelizeParams& p, int brickShape, int stackEntries, hipStream_t s);
hipError_t launch_voxelize_redo(const VoxelizeParams& p, hipStream_t s);   // finishes the rays on p.redo with a full-depth stack
int stack_round_up(int want);
int stack_for_brick(int brickShape, int want);   // the column depth compiled for this brick shape that is >= want
int num_brick_shapes();

// plan_bricks.hip -- the work queue of the lists kernel
// header of a queue: 64 heads (eight per queue: head h of queue x hands out the slots k = h mod 8 of that queue; head
// number 8 x + h), then the eight lengths, every word in a 256-byte line of its own.  Queue memory of a frame: TWO headers, then
// the slots: a launch that builds a queue takes the header the last build did not use -- all zero, because that build's
// k_plan_bricks cleared it (and the allocation cleared both) -- so no memset stands between a launch and its queue build.
// A queue is filled from both ends: the bricks that can look into a long list (dm_box_max_count: the few that take several times
// the mean) from slot 0 upwards, all others from slot cap - 1 downwards; its items are numbered heavy first (queue_slot), so a
// launch starts with its long bricks and ends with ordinary ones.  Header words per queue: eight heads, the number of heavy and
// the number of light bricks.
constexpr uint32_t kQueueHeaderWords = 5632u;
constexpr uint32_t kQueueSlotsAt = 2u * kQueueHeaderWords;
DXV_HD constexpr uint32_t queue_head_word(uint32_t x, uint32_t h) { return 64u * (1u + 8u * x + h); }
DXV_HD constexpr uint32_t queue_len_word(uint32_t x) { return 64u * (65u + x); }      // light bricks of queue x
DXV_HD constexpr uint32_t queue_heavy_word(uint32_t x) { return 64u * (73u + x); }    // heavy bricks of queue x (the sixteen words lie behind one another: one copy for dxv_sync)
DXV_HD constexpr uint32_t queue_slot(uint32_t k, uint32_t heavy, uint32_t cap) { return k < heavy ? k : cap - 1u - (k - heavy); }   // item k of a queue
// work queue of the lists kernel with 4 x 4 x 4 bricks: built on the device in front of the launch
uint32_t plan_layout(VoxelizeParams& p);           // fills the brick-order fields for the whole partition, returns its bricks
uint32_t plan_region_bits(uint32_t N, uint32_t nz); // the run length (log2 bricks) a partition of this size deals to its queues
size_t plan_queue_words(uint32_t N, uint32_t nz, uint32_t* capOut);     // 32-bit words of queue memory for a partition; *capOut = words per XCD queue
hipError_t plan_build(const VoxelizeParams& p, hipStream_t s);          // k_plan_bricks into the (zero) header p.queue; p.queueSlots, p.queueCap, p.mip set
size_t plan_live_words(uint32_t N, uint32_t nz);   // 32-bit words of a partition's brick mask
hipError_t plan_clear_grid(const VoxelizeParams& p, hipStream_t s);     // zeros the partition's grid (and texel image): the clear of k_plan_bricks as a kernel of its own
// queue_order.hip -- the direction-major order of a PREPARED queue: the bricks k_plan_bricks queued, sorted by (class, direction tile,
// start radius), whole tiles dealt round-robin to the eight queues.  Two steps around ONE read of the sixteen new counts by the caller
// (a queue must be able to hold what the deal gives it): sort -- p.queueSlots / p.queueCap / lens16 = the queue as built, n (> 0) its
// bricks, scratch = queue_order_scratch_bytes(n) bytes; *sorted and *counts (sixteen words: the heavy bricks of the eight new queues,
// then the others) point into the scratch -- and write -- p.queue = a zero header, p.queueSlots / p.queueCap = where the queues go,
// lens16 = the NEW eight lengths, of which heavy.
size_t queue_order_scratch_bytes(uint32_t n);
hipError_t queue_order_sort(const VoxelizeParams& p, const uint32_t lens16[16], uint32_t n, uint8_t* scratch, const uint64_t** sorted, const uint32_t** counts, hipStream_t s);
hipError_t queue_order_write(const VoxelizeParams& p, const uint32_t lens16[16], uint32_t n, const uint64_t* sorted, hipStream_t s);
// (test hook: out[0] items, out[1] tiles in more than one queue's own share, out[2] neighbours out of order; tiles: queue_order_check_words() words)
size_t queue_order_check_words();
hipError_t launch_queue_order_check(const VoxelizeParams& p, uint32_t* tiles, unsigned long long* out, hipStream_t s);
// voxelize_lists.hip -- the two brick kernels that run the queue
// rebuild: grid cleared + queue built in front of the kernel; else only the queue heads are reset (same launch as before into the same buffers)
// (planEvents: two events recorded around the queue build of a rebuilding launch, or NULL)
// listedLens: the eight lengths of a kept queue and how many of each are heavy (16 words) as the host last read them (one workgroup per item, dealt out by the hardware), or NULL (persistent waves)
// What the runtime answered about the two brick kernels on a context's device (persistent waves the device holds at once without / with the
// texel image; the LDS pad that holds k_voxelize_listed at 8 .. 32 workgroups per CU, -1: none).  0 = not asked yet; kept by the context,
// filled by the launchers at first use.
struct ListsOccupancy { uint32_t queueWaves[2] = {0, 0}; int listedPad[33] = {}; };
hipError_t launch_voxelize_queue(const VoxelizeParams& p, ListsOccupancy& occ, bool rebuild, uint32_t* wavesOut, hipEvent_t* planEvents, const uint32_t* listedLens, hipStream_t s);
// A launch through a queue that was PREPARED for (lists, grid, partition) -- built ONCE, in Init or by dxv_prepare_launch, like the lists
// it is a pure function of: the host knows the sixteen counts, so the hardware deals the bricks out (k_voxelize_listed, one workgroup
// per queued brick), and the grid is cleared inside the launch.  p.queueSlots / p.queueCap: the prepared queue's; lens: its sixteen
// counts (eight lengths, of which heavy); live: its bit per brick (NULL: clearMode 0).
//   clearMode 0: a kernel of its own clears the whole grid (16-byte non-temporal stores) in front of the brick kernel;
//             1 / 2 / 3: ONE dispatch -- workgroups in front of (1), behind (2) or spread evenly between (3) the bricks' zero exactly the
//             bricks that are not queued (every voxel is written once per launch, by the brick that owns it or by the clear; needs
//             N % 16 == 0).
hipError_t launch_voxelize_prepared(const VoxelizeParams& p, ListsOccupancy& occ, const uint32_t lens[16], const uint32_t* live, int clearMode, uint32_t* wavesOut, hipStream_t s);

// parity_rows.hip
hipError_t launch_parity_rows(const VoxelizeParams& p, int rowBlock, hipStream_t s);   // parity mode: one walk per row run (1) or per 2 x 2 rows (2)

// grid_utils.hip
hipError_t launch_count(const uint8_t* grid, size_t n, unsigned long long* out, hipStream_t s);
hipError_t launch_checksum(const void* buf, size_t bytes, unsigned long long* out, hipStream_t s);   // wrapping sum of the buffer's 64-bit words
hipError_t launch_pack_bits(const uint8_t* grid, size_t n, uint8_t* packed, hipStream_t s);

// surface.hip -- the surface rule (dxv_surface.h) scattered over a partition: every voxel it accepts is set to 1, nothing else is
// written (mode 2 clears the partition in front of it, mode 3 runs it behind the reference rule's launch)
struct SurfaceParams {
    const TriPos* triPos;   // T
    uint32_t T;
    uint8_t* grid;          // N*N*nz bytes
    uint32_t N, z0, nz;     // slices as VoxelizeParams: global slice of lz = z0 + (lz / zBlock) * zPeriod + lz % zBlock
    uint32_t zBlock, zPeriod;
    uint8_t* scratch;       // surface_scratch_bytes(T): the large triangles' lists and counters (one per frame: frames run side by side)
    uint32_t items;         // work items the list may take: 0 = all it holds (2^20); fewer: option surfaceitems (tests)
};
size_t surface_scratch_bytes(uint32_t T);
hipError_t launch_surface(const SurfaceParams& p, hipStream_t s);

// distance.hip -- the exact signed distance field of a whole N^3 grid (dxv_distance.h): format 0 = int32 s * d2, 1 = float32 s * sqrt(d2);
// field: 4 * N^3 bytes, scratch: distance_scratch_bytes(N) (dxv_distance.h); grid, field and scratch are three different allocations
hipError_t launch_distance(const uint8_t* grid, uint32_t N, int format, void* field, uint8_t* scratch, hipStream_t s);

// fill.hip -- the exterior flood fill of a whole N^3 grid (dxv_fill.h), in place: one batch = (first: the grid packed into the free and
// reached masks,) `rounds` rounds (1 .. kFillMaxRounds), the write-back of what = 0 (walls and what they enclose) or 1 (the enclosed voxels
// alone).  scratch: fill_carve (dxv_fill.h), the two masks and the batch's control block -- word k != 0: round k changed something; the
// batch has converged exactly when the word of its last round is 0.  A batch with first = false goes on from the masks of the one before.
struct FillScratch;
hipError_t launch_fill(uint8_t* grid, uint32_t N, int what, const FillScratch& scratch, uint32_t rounds, bool first, hipStream_t s);

// mesh_distance.hip -- the exact distance from the voxel centres of slices [z0, z0 + nz) of an N^3 grid to the mesh, signed by the grid's
// bytes (dxv_mesh_distance.h): walk = the nearest-triangle query over the two-box nodes (a tree no higher than kMdStack), else every
// triangle for every voxel.  field: 4 bytes per voxel, element ((iz - z0) * N + iy) * N + ix like the grid; tris: the same, or null.
struct MeshDistanceParams {
    const uint8_t* grid;
    float* field;
    uint32_t* tris;         // tri(p), or null: not wanted
    uint32_t N, z0, nz;
    int format;             // DXV_MDIST_VOXELS_F32 / DXV_MDIST_UNITS_F32
    float cap;              // md_cap(N, band): what every minimum starts from
    float cullAbs;          // md_cull_abs(root box)
};
hipError_t launch_mesh_distance(const Node* nodes, const TriPos* triPos, uint32_t T, const MeshDistanceParams& p, bool walk, hipStream_t s);

// scan.hip -- the exclusive scan of the grid operators (dxv_scan.h has the workgroup's routine).  launch_scan_words: `words` words of C (1 or 2)
// interleaved 32-bit counts each become what stands in front of them, in place; sums: C * scan_blocks(words) (dxv_scratch.h) 64-bit words of scratch; totals: C
// 64-bit words.  launch_scan_sums: the same for `blocks` entries of C 64-bit sums, by one workgroup; totals may stand right behind them.  Both
// refuse a null pointer, a C that is neither 1 nor 2, and nothing to scan.
hipError_t launch_scan_words(uint32_t* counts, uint32_t C, size_t words, unsigned long long* sums, unsigned long long* totals, hipStream_t s);
hipError_t launch_scan_sums(unsigned long long* sums, uint32_t C, uint32_t blocks, unsigned long long* totals, hipStream_t s);

// isosurface.hip -- a triangle mesh from a float32 field of a whole N^3 grid by naive Surface Nets (dxv_isosurface.h): count + scan, ONE
// read of the two totals by the caller, emit.  scratch: iso_carve (dxv_isosurface.h).  vb: 24 bytes per vertex, ib: three uint32 per triangle, two
// triangles per quad.
struct IsoParams;
hipError_t launch_iso_count(const IsoParams& p, hipStream_t s);
hipError_t launch_iso_emit(const IsoParams& p, hipStream_t s);

// octree.hip -- the sparse voxel octree of a whole N^3 grid (dxv_octree.h): reduce + scan, ONE read of the L + 1 level totals by the caller,
// emit; and the way back, a grid from a tree.  scratch: oct_carve (dxv_octree.h).  nodes: 8 bytes each.
struct OctParams;
hipError_t launch_oct_count(const OctParams& p, hipStream_t s);
hipError_t launch_oct_emit(const OctParams& p, hipStream_t s);
// every voxel of the grid of side N becomes 0 or 1 from a tree of `count` nodes (4-byte aligned, not trusted); *bad = 1 if it cannot be followed
hipError_t launch_oct_expand(uint8_t* grid, uint32_t N, const uint32_t* nodes, uint32_t count, uint32_t* bad, hipStream_t s);

// components.hip -- the connected components of a whole N^3 grid (dxv_components.h): pack, init, merge, compress, number; ONE read of K by the
// caller; the table.  scratch: comp_carve (dxv_components.h).  labels: N^3 uint32; table: 24 bytes per component; stats: 32 bytes per component
// of work.
struct CompRecord;
struct CompParams;
struct CompSelectWork;
hipError_t launch_comp_label(const CompParams& p, hipStream_t s);
hipError_t launch_comp_stats(const CompParams& p, uint32_t K, hipStream_t s);
// dxv_components_select: `work` -- comp_select_carve -- holds {kept, dropped, voxels changed, the maximum of comp_best_key}, then K keep flags
hipError_t launch_comp_select(uint8_t* grid, uint32_t N, int of, const uint32_t* labels, const CompRecord* table, uint32_t K, int rule, uint32_t arg,
                              const CompSelectWork& work, hipStream_t s);
// ... its pack alone: grid -> the member mask (the first block of the scratch), for what reads the mask of a labelling after dxv_trim
hipError_t launch_comp_pack(const uint8_t* grid, uint32_t N, int of, uint64_t* mask, hipStream_t s);
// ... and its merge and its compress alone, for an operator that labels masks of its own over a parent array it has initialised (skeleton.hip)
hipError_t launch_comp_merge(const uint64_t* mask, uint32_t N, uint32_t connectivity, uint32_t* parent, hipStream_t s);
hipError_t launch_comp_compress(uint32_t* parent, uint32_t N, hipStream_t s);

// skeleton.hip -- the skeleton graph of a whole N^3 grid (dxv_skeleton.h): pack, classify, init, merge and compress (the components'), number; ONE
// read of {K, B} by the caller; the tables.  scratch: skel_carve (dxv_skeleton.h).  labels: N^3 uint32; nodes: 32 bytes each; branches: 48 bytes
// each; stats: 40 bytes per node of work.  The grid is only read.
struct SkelNode;
struct SkelBranch;
struct SkelParams;
struct SkelPruneWork;
hipError_t launch_skel_classify(const SkelParams& p, hipStream_t s);
hipError_t launch_skel_label(const SkelParams& p, hipStream_t s);
hipError_t launch_skel_stats(const SkelParams& p, uint32_t K, uint32_t B, hipStream_t s);
// dxv_skeleton_prune: `work` -- skel_prune_carve -- holds {branches removed, voxels removed}, then a flag per branch and per node
hipError_t launch_skel_prune(uint8_t* grid, uint32_t N, const uint32_t* labels, const SkelNode* nodes, uint32_t K, const SkelBranch* branches, uint32_t B, uint32_t maxLen345,
                             const SkelPruneWork& work, hipStream_t s);

// measure.hip -- the integral measures of the K components of a labelling (dxv_measure.h): table = measure_table_bytes(K) = (K + 1) * 96 bytes,
// record 0 the sum of the others; mask: the labelling's member mask; labels: N^3 uint32.  Nothing but the table is written.
size_t measure_table_bytes(uint32_t K);
hipError_t launch_measure(const uint64_t* mask, uint32_t N, uint32_t connectivity, const uint32_t* labels, uint32_t K, uint8_t* table, hipStream_t s);

// morph.hip -- DILATE / ERODE / OPEN / CLOSE (0 .. 3) of a whole N^3 grid by the Euclidean ball of squared radius r2 (1 .. 4096; dxv_morph.h), in
// place, bytes 0 / 1.  form 1: word-parallel on bit masks and R = floor(sqrt(r2)) planes; form 2: the distance field and its threshold, per
// half.  scratch: morph_carve(N, op, r2, form) (dxv_morph.h); it begins with {voxels set, voxels cleared}
struct MorphScratch;
hipError_t launch_morph(uint8_t* grid, uint32_t N, int op, uint32_t r2, int form, const MorphScratch& scratch, hipStream_t s);
// ... its pack (grid -> the solid mask and the "a byte here is neither 0 nor 1" bits, one per eight voxels) and its write-back (was, now: the solid
// masks before and after; counters: {voxels set, voxels cleared}, added to) for the operators that work on the same masks
void launch_morph_pack(const uint8_t* grid, uint32_t N, uint8_t* mask, uint64_t* loose, hipStream_t s);
void launch_morph_write(const uint8_t* was, const uint8_t* now, const uint64_t* loose, uint32_t N, uint8_t* grid, unsigned long long* counters, hipStream_t s);

// thin.hip -- topology-preserving thinning of a whole N^3 grid (dxv_thin.h), kind 0 = CURVE, 1 = KERNEL, in place, bytes 0 / 1: one batch =
// (first: the grid packed into the solid mask,) `iterations` iterations (1 .. kThinMaxRounds) of border + eight sub-iterations, the write-back.
// scratch: thin_carve (dxv_thin.h); it begins with the batch's control block -- word k != 0: iteration k removed something; the batch has reached
// the fixed point exactly when one of its words is 0 -- and the voxels removed since the first batch.  A batch with first = false goes on from
// the masks of the one before.
struct ThinScratch;
hipError_t launch_thin(uint8_t* grid, uint32_t N, int kind, const ThinScratch& scratch, uint32_t iterations, bool first, hipStream_t s);

// thickness.hip -- the exact local thickness of a whole N^3 grid (dxv_thickness.h): W = N^3 uint32, hist = cap + 1 uint64, both the caller's;
// everything else in scratch, laid out by thickness_carve (dxv_thickness.h, with ThickParams).  Six stages, enqueued one by one so that the caller
// can put its events between them; nothing is read back: p.counters points at {centres painted, work items, voxels the paint tested, atomics it
// sent} in the scratch, the first two valid behind the select.  The grid is only read.
struct ThickParams;
enum { THICK_STAGE_FIELD, THICK_STAGE_TOP, THICK_STAGE_CULL, THICK_STAGE_SELECT, THICK_STAGE_PAINT, THICK_STAGE_HISTOGRAM, THICK_STAGES };
size_t thickness_histogram_bytes(uint32_t cap);
hipError_t launch_thickness_stage(const uint8_t* grid, const ThickParams& p, int stage, hipStream_t s);

// partition.hip -- the maximal-ball partition of a whole N^3 grid (dxv_partition.h): labels = N^3 uint32, table = 32 K bytes, throats = 20 T bytes,
// all the caller's.  scratch is laid out by partition_carve, work by partition_work_carve (dxv_partition.h, with PartParams) once the caller has
// waited for p.totals = {K, interface faces} behind PART_STAGE_ROOTS.  The stages are enqueued one by one so that the caller can put its events
// between them; the throats take launch_partition_pairs, a wait for p.pairTotal = T, and launch_partition_throats.  p.counters points at {mip
// cells tested, voxels tested} of the search (option partstages).  The grid is only read.
struct PartParams;
enum { PART_STAGE_FIELD, PART_STAGE_KEYS, PART_STAGE_SEARCH, PART_STAGE_ROOTS, PART_STAGE_REGIONS, PART_STAGE_THROATS, PART_STAGES };
hipError_t launch_partition_stage(const uint8_t* grid, const PartParams& p, int stage, hipStream_t s);     // PART_STAGE_FIELD .. PART_STAGE_REGIONS
hipError_t launch_partition_pairs(PartParams& p, hipStream_t s);
hipError_t launch_partition_throats(const PartParams& p, uint32_t T, uint32_t* throats, hipStream_t s);

// geodesic.hip -- the geodesic distance inside a whole N^3 grid (dxv_geodesic.h): map = N^3 uint32, the caller's; everything else in scratch =
// geodesic_carve (dxv_geodesic.h, with GeoControl): the batch's control block -- word k = the live tiles of round k; the batch has reached the fixed
// point exactly when one of its words is 0 --, the tally {seeds used, reached, unreached, key}, two sets of live flags (a byte per 8^3 tile) and
// the queue (a word per tile).  launch_geodesic_init: the map's first words and the live flags of round 0 from the grid and the seeds -- `seeds`
// is a device pointer, N^3 bytes for GEO_SEEDS_MASK, seedCount voxel indices for GEO_SEEDS_LIST.  launch_geodesic_batch: `rounds` rounds
// (1 .. kGeoMaxRounds), the first of them round `base` of the call, then the tally.  The grid is read by the init alone.
struct GeoControl;
struct GeoScratch;
hipError_t launch_geodesic_init(const uint8_t* grid, uint32_t N, int of, int seedsKind, const void* seeds, uint32_t seedCount, uint32_t* map, const GeoScratch& scratch,
                                hipStream_t s);
hipError_t launch_geodesic_batch(uint32_t* map, uint32_t N, int metric, uint32_t limit, const GeoScratch& scratch, uint32_t rounds, uint32_t base, hipStream_t s);
// ... and the path from `target` down to a seed, by one wave: out = {voxels on the path, 0 or 1: no neighbour continued it}, then min(length,
// capacity) voxel indices
hipError_t launch_geodesic_path(const uint32_t* map, uint32_t N, int metric, uint32_t target, uint32_t* out, uint32_t capacity, hipStream_t s);
// ... and the compaction of a round's live flags alone, for an operator with flags, queue and control block of the same shape (access.hip)
hipError_t launch_geodesic_compact(uint8_t* live, uint32_t tiles, GeoControl* ctl, uint32_t round, uint32_t* queue, hipStream_t s);

// access.hip -- the access radius inside a whole N^3 grid and its intrusion map (dxv_access.h): A = N^3 uint32, the caller's, and with
// `intrusion` I likewise; the histograms cap + 1 uint64 each; everything else in scratch, laid out by access_carve (dxv_access.h): a control block,
// live flags and a queue of the geodesic's shape, the word the seeds are counted in, and behind them the radius field F with the scratch of its
// passes -- with `intrusion` the whole of a thickness's scratch, which begins with F.  launch_access_init: the field, A's first words and the live
// flags of round 0.  launch_access_batch: `rounds` rounds (1 .. kAccMaxRounds), the first of them round `base` of the call, then the tally.
// launch_access_radius, once A has settled: A into F in thick_radius's encoding, for launch_thickness_stage TOP .. HISTOGRAM with W = I.  The grid
// is read by the field alone.
struct AccScratch;
hipError_t launch_access_init(const uint8_t* grid, uint32_t N, int of, uint32_t cap, int seedsKind, const void* seeds, uint32_t seedCount, uint32_t* A, const AccScratch& scratch,
                              hipStream_t s);
hipError_t launch_access_batch(uint32_t* A, uint32_t N, int of, int connectivity, uint32_t cap, const AccScratch& scratch, uint32_t rounds, uint32_t base, hipStream_t s);
hipError_t launch_access_radius(const uint32_t* A, uint32_t N, int of, const AccScratch& scratch, hipStream_t s);

// sight.hip -- the line-of-sight map of a whole N^3 grid (dxv_sight.h): map = N^3 uint32, the caller's; everything else in scratch, laid out by
// sight_carve (dxv_sight.h): the tally's 68 words, the member mask and one bit plane per requested direction.  launch_sight: pack, ONE sweep launch
// for all directions, the map, the tally; group = option sightgroup (0: the smallest row group).  The grid is read by the pack alone.
// launch_sight_fill: the edit from a map -- every member of the map's kind whose word shares no bit with `directions` changes kind, in place.
struct SightScratch;
hipError_t launch_sight(const uint8_t* grid, uint32_t N, int of, uint32_t directions, uint32_t group, uint32_t* map, const SightScratch& scratch, hipStream_t s);
hipError_t launch_sight_fill(uint8_t* grid, uint32_t N, int of, uint32_t directions, const uint32_t* map, hipStream_t s);

// raycast.hip
struct RayCastCB;
hipError_t launch_raycast(const RayCastCB& cb, const uint8_t* grid, uint32_t N, uint32_t width, uint32_t height,
                          uint8_t* rgba8, size_t pitch, uint8_t* empty, hipStream_t s);
size_t empty_brick_bytes(uint32_t N);

} // namespace dxv
