// dxv_policy.h -- the decisions of the host side as pure functions of plain state: WHEN the candidate lists of the reference rule
// are built and on WHICH cube map, and whether a launch builds its work queue, keeps it, or has the hardware deal it out.
// dxv_lists.hip / dxv_frames.hip carry the decisions out; tests/hostcheck compiles this header for the CPU and
// tests/test_policy.py walks every transition (static scene, dynamic scene, the C-ABI's own rules, options) as a table.
// The options of dxv_set_option are a table here as well: what each key accepts and where its value lives.
// No HIP, no context: nothing here touches a device.
#pragma once
#include <stdint.h>
#include <string.h>

namespace dxv {

// ---------------------------------------------------------------------------------------------
// lists: state of a scene's direction-space lists as the host sees it in front of a reference-rule launch
// ---------------------------------------------------------------------------------------------
struct ListsState {
    int optLists;            // option lists: 0 tree walk, 1 by the rules below, 2 from the first launch
    int optListRes;          // option listres: 0 automatic, else the map asked for
    int listOpt;             // the listres option the current lists (or the decision against them) were made with
    int listState;           // 0 not built for this scene, 1 built, -1 over the caps (tree walk)
    uint32_t listRes;        // map of the lists there are
    uint64_t listEntries;
    uint32_t numTris;
    uint32_t launchesOfScene; // reference-rule launches since the scene last changed (build / refit / import)
    bool refitted;           // dxv_refit has run since dxv_build: the mesh is being animated
    bool floorTried;         // the move to the fine map has been made (or tried) for this scene
};
constexpr uint32_t kListsFineMap = 512u;          // the map of a static scene of kListsFineFrom triangles or more
constexpr uint32_t kListsFineFrom = 20000u;
constexpr uint64_t kListsPayFromVoxels = 1ull << 26;   // a FIRST launch of this size may build its lists at once (when the build's estimate agrees)

// base map by triangle count (5 - 10 entries per texel: coarser maps have long lists, finer ones stop fitting the caches)
inline uint32_t lists_base_map(uint32_t numTris, int optListRes)
{
    if (optListRes) return (uint32_t)optListRes;
    return numTris < kListsFineFrom ? 128u : numTris < 3000000u ? 256u : 512u;
}
// deep scenes (over 32 entries per texel: soups) keep coarse maps -- what matters there is the size of the structure
inline bool lists_deep(uint64_t entries, uint32_t R) { return (double)entries > 32.0 * 6.0 * (double)R * (double)R; }

// What to do to the lists in front of a launch of `voxels` voxels (relaunch: the same launch again with a deeper column or after
// withdrawn lists -- it builds nothing).  At most one build per call; the caller applies it, updates the state and asks
// lists_used.
enum class ListsStep {
    none,
    build_if_it_pays,        // a scene's FIRST launch under lists = 1, large enough: count, estimate, build on the base map or decline
    move_to_fine_map,        // lists on a coarser map and the scene is launched AGAIN without a refit in between: a static scene -- once, the 512 map
    build                    // lists wanted and not there (or made for another listres option)
};
inline ListsStep lists_step(const ListsState& s, uint64_t voxels, bool relaunch)
{
    if (relaunch || !s.optLists) return ListsStep::none;
    if (s.optLists == 1 && s.launchesOfScene == 0 && s.listState == 0 && voxels >= kListsPayFromVoxels) return ListsStep::build_if_it_pays;
    if (!s.optListRes && s.listState == 1 && s.listRes < kListsFineMap && !s.refitted && !s.floorTried && s.launchesOfScene > 0 &&
        s.numTris >= kListsFineFrom && !lists_deep(s.listEntries, s.listRes))
        return ListsStep::move_to_fine_map;
    const bool want = s.optLists == 2 || s.launchesOfScene > 0 || s.listState != 0;
    if (want && (s.listState == 0 || s.listOpt != s.optListRes)) return ListsStep::build;
    return ListsStep::none;
}
// ... and whether the launch then goes through the lists (state after the step has been applied)
inline bool lists_used(const ListsState& s, bool relaunch)
{
    if (!s.optLists || s.listState != 1) return false;
    if (relaunch) return s.listOpt == s.optListRes;
    return s.optLists == 2 || s.launchesOfScene > 0 || s.listState != 0;
}
// dxv_build_lists_for_grid (what Init of the host mirrors calls for a static scene): straight to the fine map?
inline bool lists_static_scene_takes_fine_map(const ListsState& s, uint32_t floorNow)
{
    return !s.optListRes && s.numTris >= kListsFineFrom && !s.refitted && !s.floorTried && floorNow < kListsFineMap;
}

// The map a build settles on once the counting pass has said how many entries the map it counted on would hold (0: keep it).
//   oneLaunch: the build must pay for itself on one launch (a first-launch build, a mesh that is being refitted): base map
//   coarser: this count was already a step down from a finer map (a deep scene): only further down from here
inline uint32_t lists_recount_on(uint32_t R, uint64_t entries, bool oneLaunch, int optListRes, bool coarser)
{
    if (optListRes) return 0u;
    if (!coarser && !oneLaunch && R == 256u && !lists_deep(entries, R)) return kListsFineMap;   // a static scene: the fine map beats the 256 map at every grid size
    if (coarser ? R == 256u : lists_deep(entries, R)) {
        if (R != 256u) return 256u;
        if (entries > (320ull << 20)) return 128u;
    }
    return 0u;
}
// a build of this many triangles counts every kListsSampleStride-th of them first and lets the estimate pick the map
constexpr uint32_t kListsSampleFrom = 3000000u, kListsSampleStride = 16u;
inline bool lists_sample_first(uint32_t numTris, int optListRes) { return !optListRes && numTris >= kListsSampleFrom; }
// scenes whose lists would exceed 256 entries per triangle + 64 M, or 2^31, keep the tree walk
inline bool lists_over_the_caps(uint64_t entries, uint32_t numTris) { return entries > 256ull * numTris + (64ull << 20) || entries > 0x7fffffffull; }
// a first-launch build goes on only when what the lists save on THIS launch exceeds what the rest of the build costs
inline bool lists_pay_on_first_launch(uint64_t voxels, uint64_t entries, uint32_t R)
{
    const double perTexel = (double)entries / (6.0 * R * R), depth = perTexel > 10.0 ? perTexel / 10.0 : 1.0;
    return (double)voxels * 1e-8 * depth >= 0.1 + 0.15e-6 * (double)entries;
}

// ---------------------------------------------------------------------------------------------
// far-radius map of a scene WITHOUT lists (the brick test of its tree walks, dirmap_far): made when the scene is launched over the brick
// box a SECOND time without having changed -- a mesh refitted every frame never pays 0.13 ms (1 M triangles) for a map that one
// launch would read and that saves that launch 1 - 5 %
// ---------------------------------------------------------------------------------------------
inline bool far_map_build_now(bool haveForScene, uint32_t boxLaunchesOfScene) { return !haveForScene && boxLaunchesOfScene >= 1u; }

// ---------------------------------------------------------------------------------------------
// work queue: what a launch through the lists does about its queue
// ---------------------------------------------------------------------------------------------
struct QueueState {
    int optPlan;             // 2 every launch builds (default), 1 kept while the launch is the same, (0: no queue -- not asked here)
    int optDispatch;         // a kept queue of known size: 1 dealt out by the hardware, 2 only for partitions of up to 2^25 voxels, 0 never
    bool ptrExposed;         // the caller holds a writable pointer to the frame's grid
    uint64_t keptSig;        // signature of the launch whose queue and zeros the frame still carries (0: none)
    uint64_t lensSig;        // signature of the queue whose lengths a dxv_sync has read (0: none)
    uint32_t queuedBricks;   // ... their sum
    int optPrepared;         // 1: launches of a prepared partition use its queue
    bool prepared;           // the context holds a queue PREPARED for this launch's (lists, grid, partition, queue options)
};
// Persistent waves of a launch through the queue, in sevenths of what the device holds at once (7 waves per SIMD).  A brick of a
// coarse grid looks into a large patch of the map (5.6 R / N texels across), and on a mesh of many small triangles the rays of
// one brick meet dozens of different triangles: seven such waves per SIMD get in each other's way in the vector caches, five or four
// finish the launch sooner (256^3 on the 512 map, nothing carried: torus-1M 0.190 -> 0.166 ms, bunny x16 0.217 -> 0.183, dragon x9
// 0.145 -> 0.138; 128^3: 0.069 -> 0.064 with four).  Meshes of few triangles lose (bunny 256^3: +5 % with five), and so does every
// mesh on a grid as fine as the map (512^3: +12 %): all waves there.  (profiles/r05/ab_waves_by_grid.jsonl; option queuewaves
// overrides.)
constexpr uint32_t kQueueFineMeshFrom = 500000u;
inline uint32_t queue_waves_sevenths(uint32_t numTris, uint32_t R, uint32_t N)
{
    if (numTris < kQueueFineMeshFrom) return 7u;
    if (4ull * N <= R) return 4u;
    if (2ull * N <= R) return 5u;
    return 7u;
}
// prepared_hardware: the queue came from Init (dxv_prepare_launch); the launch clears its grid and the hardware deals the bricks out --
// nothing of the OUTPUT is carried, and what is read (the queue) is structure of the static scene like the lists.  It wins over a
// kept queue (plan = 1) too: same kernel, and no dependence on the frame's last launch.
enum class QueueLaunch { build_and_persistent, kept_persistent, kept_hardware, prepared_hardware };
inline QueueLaunch queue_policy(const QueueState& q, uint64_t sig, uint64_t voxels)
{
    if (q.prepared && q.optPrepared && q.optPlan != 0) return QueueLaunch::prepared_hardware;
    if (q.optPlan == 2 || q.ptrExposed || q.keptSig != sig) return QueueLaunch::build_and_persistent;
    const bool sizeKnown = q.lensSig == sig && q.queuedBricks != 0u;
    if (sizeKnown && (q.optDispatch == 1 || (q.optDispatch == 2 && voxels <= (1ull << 25)))) return QueueLaunch::kept_hardware;
    return QueueLaunch::kept_persistent;
}

// Do the launches through the lists read the start table?  The word is one more load per ray in a kernel bound by the number of its
// load instructions, and the brick kernels compiled with the table are 5 - 6 % slower than the plain ones before the table saves
// anything (voxelize_lists.hip keeps both forms): it pays where it removes whole scan rounds from most waves, and a wave is as slow as
// its worst lane.  What decides is how many texels hold more than 8 entries -- the lists the start search leaves a whole window of
// entries in front of a ray in: at least a third of the non-empty texels (counted by the table's build).  Measured, table kernels with
// the table against plain kernels, ms per prepared launch (profiles/start_table/option_ab_final_kernels.jsonl): torus-1M, 50 % of the
// non-empty texels, 0.553 -> 0.518 (-6 %); dragon x9 at 1024^3, 16 %, 2.029 -> 2.086 (+3 %); bunny x16, 8 %, 0.602 -> 0.641 (+6 %) --
// a line through the first two crosses zero at 28 %.  Option starttable: 0 / 1 as asked, 2 = by this rule.
inline bool start_table_pays(uint32_t nonEmptyTexels, uint32_t texelsOver8) { return nonEmptyTexels != 0u && 3ull * texelsOver8 >= nonEmptyTexels; }
inline bool start_table_used(int optStartTable, bool pays) { return optStartTable == 1 || (optStartTable == 2 && pays); }

// ---------------------------------------------------------------------------------------------
// options (dxv_set_option; include/dxv.h documents what they do): the values a context holds, and one row per key -- its name, the
// values it accepts, the words a refusal ends in, where the value is stored and whether setting it does more than store it
// (dxv_api.hip carries those few out).  tests/test_policy.py checks every row against expectations written out there.
// ---------------------------------------------------------------------------------------------
struct Options {
    int brick = 4;           // 4x4x4 voxels = one wavefront per workgroup (fastest in the r01 sweeps)
    int stack = 0;           // 0 = adaptive (start small, grow on overflow), else forced depth
    int deferboxes = 1;      // dxv_refit with lists wanted: node boxes only when a tree walk asks for them (0: always, as dxv_build does)
    int refit = 1;           // box merge of build and refit: 1 = min/max pyramid (default), 2 = level sweeps, 0 = atomic one-pass climb (17-30x slower, cross-check)
    int morton = 1;          // Morton brick order
    int queue = 1;           // postponed-leaf traversal
    int subbox = 1;          // launch only the bricks around the scene's root box, memset the rest
    int wide = 2;            // reference rule: 2 = four-box nodes on wave-uniform visits (-2...-7 % everywhere measured),
                             // 1 = on every visit (-8 % on low-poly meshes, +10 % on 1 M triangles at 256^3), 0 = binary only
    int rows = 1;            // parity mode: one tree walk per grid row (k_parity_rows) instead of per voxel
    int rowblock = 0;        // rows per side of a wave's block of rows: 0 = by triangle size, 1, 2
    int ablate = 0;          // timing-only variants of the lists kernel (results are wrong by design; tools/ablate.py)
    int region = 6;          // log2 bricks per XCD region (64 bricks: balanced and L2 friendly in the r01 sweeps)
    int stack0 = 20;         // adaptive mode starts with this many entries (stack + leaf queue share them)
    int lists = 1;           // reference rule through the lists (-40...-60 % against the tree walk, profiles/r01/final/ab_lists.jsonl):
                             // 1 = from a scene's second launch on (from the first when that launch is large: build_lists), 2 = from the first, 0 = tree walk
    int listres = 0;         // texels per face side; 0 = by triangle count (list_resolution)
    int listedwaves = 0;     // workgroups per CU of the hardware-dispatched lists kernel (8 .. 32), or 0 = by grid and map (voxelize_lists.hip: listed_lds_pad)
    int starttable = 2;      // the lists' per-texel start table (dxv_dirmap.h: dm_start_word): 0 = scans begin where the start search ends, 1 = no earlier
                             // than the table's start for the ray, 2 = automatic (default: where it pays -- start_table_pays)
    int lateralpad = 1;      // the lists' lateral dilation (dxv_dirmap.h: dm_lateral_pad): 1 = every whole, well-shaped projected triangle by its own bound, 0 = all by 2^-15.
                             // Read by the list build; a change drops lists, start table, start cells and prepared queues.  Same grids.
    int coop = 1;            // 1: the lists kernel scans a lone lane's long list with its whole wave (dxv_dirmap.h: trace_reference_dm_from)
    int farmap = 1;          // 1: tree walks and brick-box launches of the reference rule skip the bricks none of whose rays can reach a triangle
    int plan = 2;            // work queue of the lists kernel (live bricks only, built on the device inside the stream): 0 = none (brick box
                             // in Morton order), 1 = built when lists, partition or buffers differ from the frame's last launch (opt-in), 2 = on every launch (default: nothing carried)
    int queuewaves = 0;      // persistent waves of a queue launch; 0 = what the device holds at once
    int queuemin = 0;        // persistent waves: at least this many bricks per wave (surplus waves leave at once); 0 (default) = every wave stays.
                             // 12: torus-1M / bunny x16 at 256^3 -13 / -11 %, but dragon x9 +11 % at 256^3 and +35 % on a rank's share: not a
                             // rule a launch can apply blind (profiles/r05/ab_surplus_waves_leave.jsonl, short_launches_queuemin12.jsonl)
    int queueheads = 8;      // heads per queue (persistent waves): 1, 2, 4, 8
    int planregion = 0;      // log2 of the run of Morton bricks dealt to one queue: 6, 7, 8; 0 = by the partition's size (plan_region_bits)
    int planheavy = 0;       // list length beyond which a brick starts early; 0 = long for this scene (k_dm_heavy_thresholds), 65535: no brick does
    int fuse = 1;            // 1: the queue build clears the grid as well (one kernel in front of the brick kernel); 0: memsets in front of it
    int dispatch = 1;        // a kept queue whose lengths the host knows: 0 = persistent waves all the same, 1 = one workgroup per
                             // queued brick dealt out by the hardware (-1 ... -10 % per launch, and back-to-back launches overlap
                             // their ends: profiles/r04/ab_dispatch_kept_queue.jsonl), 2 = that for partitions of up to 2^25 voxels only
    int events = 1;          // bracket every launch with two HIP events (stats.voxelize_ms); 0: none (a caller timing its own loop)
    int prepared = 1;        // launches of a prepared partition use its queue (1, default); 0: they build their own like any other launch
    int prepclear = 2;       // how such a launch clears: 0 = a clear kernel in front of the brick kernel, 1 / 2 = only the bricks nobody runs,
                             // by workgroups in front of / behind the bricks' in the SAME dispatch
    int plistres = 0;        // texels per side of the row lists' grid; 0 = by triangle count
    int plists = 1;          // 1 = from a scene's second parity launch, 2 = from the first, 0 = tree walk
    int skipempty = 1;       // display pass: skip the samples of empty 8^3 bricks (same image)
    int surfaceitems = 0;    // surface modes: work items the large triangles' list may take (0: all 2^20 it holds; fewer: tests of a full list)
    int fillrounds = 0;      // dxv_fill*: rounds of one batch (1 .. 64); 0 = kFillRoundsDefault (dxv_fill.h).  Same grids: a fill that needs more is
                             // continued where its frame is next synchronised
    int thinrounds = 0;      // dxv_thin*: iterations of one batch (1 .. 64); 0 = kThinRoundsDefault (dxv_thin.h).  Same grids: a thin that needs more is
                             // continued where its frame is next synchronised
    int georounds = 0;       // dxv_geodesic*: rounds of one batch (1 .. 64); 0 = kGeoRoundsDefault (dxv_geodesic.h).  Same map: a geodesic that needs more is
                             // continued where its frame is next synchronised
    int accessrounds = 0;    // dxv_access*: rounds of one batch (1 .. 64); 0 = kAccRoundsDefault (dxv_access.h).  Same maps: an access that needs more is
                             // continued where its frame is next synchronised
    int sightgroup = 0;      // dxv_sight*: lanes of a row group of the sweep at the least (1, 2, 4, 8, 16); 0 = the next power of two >= the row's words
                             // (dxv_sight.h: sight_group).  Same map, same tally: a test reaches the widest group without a grid of 514^3
    int morphform = 0;       // dxv_morph*: 0 = by the radius (dxv_morph.h: morph_form), 1 = bit planes, 2 = distance field + threshold.  Same grids.
    int thickcull = 3;       // dxv_thickness*: bit 0 = the Top cull, bit 1 = neighbour domination (dxv_thickness.h).  Same map, same histogram.
    int thickstages = 0;     // dxv_thickness*: 1 = every stage between events of its own and the paint counts its tests and atomics (dxv_thickness_stage_info); measurement
    int partprune = 3;       // dxv_partition*: bit 0 = the 4^3 mip level of the parent search, bit 1 = the 16^3 level (dxv_partition.h); 0 = the plain ball walk.  Same bytes.
    int partstages = 0;      // dxv_partition*: 1 = every stage between events of its own and the search counts the cells and voxels it tests (dxv_partition_stage_info); measurement
    int mdistwalk = 1;       // dxv_mesh_distance*: 1 = the nearest-triangle query over the hierarchy, 0 = every triangle for every voxel (cross-check; same field)
    int sortbits = 0;        // digit plan of the radix sort as last set through this context (the plan itself is the process's: radix_sort_set_plan)
};

struct OptionRule {
    enum Kind { range, pow2, set, sortbits } kind;   // [lo, hi]; a power of two in [lo, hi]; a member of `members`; sortbits' own
    bool orZero;                                     // ... or 0
    int64_t lo, hi;
    int64_t members[11];                             // (set: ended by -1)
};
constexpr OptionRule in_range(int64_t lo, int64_t hi) { return {OptionRule::range, false, lo, hi, {}}; }
constexpr OptionRule zero_or_range(int64_t lo, int64_t hi) { return {OptionRule::range, true, lo, hi, {}}; }
constexpr OptionRule zero_or_pow2(int64_t lo, int64_t hi) { return {OptionRule::pow2, true, lo, hi, {}}; }
template <class... V> constexpr OptionRule one_of(V... v) { return {OptionRule::set, false, 0, 0, {(int64_t)v..., -1}}; }
constexpr OptionRule kOnOff = in_range(0, 1);
constexpr OptionRule kSortBits = {OptionRule::sortbits, false, 0, 63, {}};    // 0 or 8..11 bits per digit, + 16 / + 32 / + 48

// what dxv_set_option does for a key beyond checking and storing its value
enum class OptionEffect { none, brick, wide, listres, plistres, stack0, sortbits, ablate, lateralpad };
struct OptionRow { const char* name; OptionRule rule; const char* refusal; int Options::*where; OptionEffect effect; };

// (stack, stack0: the column depths the brick kernels are compiled for -- stack_round_up, traverse.hip)
constexpr OptionRow kOptions[] = {
    {"brick", in_range(0, 7), "out of range", &Options::brick, OptionEffect::brick},          // (... and below num_brick_shapes())
    {"stack", one_of(0, 8, 12, 16, 20, 24, 32, 48, 64), "not in {0,8,12,16,20,24,32,48,64}", &Options::stack, OptionEffect::none},
    {"refit", in_range(0, 2), "not in {0,1,2}", &Options::refit, OptionEffect::none},
    {"deferboxes", kOnOff, "not in {0,1}", &Options::deferboxes, OptionEffect::none},
    {"subbox", kOnOff, "not in {0,1}", &Options::subbox, OptionEffect::none},
    {"wide", in_range(0, 2), "not in {0,1,2}", &Options::wide, OptionEffect::wide},
    {"lists", in_range(0, 2), "not in {0,1,2}", &Options::lists, OptionEffect::none},
    {"plan", in_range(0, 2), "not in {0,1,2}", &Options::plan, OptionEffect::none},
    {"prepared", kOnOff, "not in {0,1}", &Options::prepared, OptionEffect::none},
    {"listedwaves", zero_or_range(8, 32), "not in {0,8..32}", &Options::listedwaves, OptionEffect::none},
    {"coop", kOnOff, "not in {0,1}", &Options::coop, OptionEffect::none},
    {"farmap", kOnOff, "not in {0,1}", &Options::farmap, OptionEffect::none},
    {"prepclear", in_range(0, 3), "not in {0,1,2,3}", &Options::prepclear, OptionEffect::none},
    {"queuewaves", in_range(0, 1 << 20), "not in [0, 2^20]", &Options::queuewaves, OptionEffect::none},
    {"queuemin", in_range(0, 4096), "not in [0, 4096]", &Options::queuemin, OptionEffect::none},
    {"sortbits", kSortBits, "not 0 or 8..11 (+16 / +32)", &Options::sortbits, OptionEffect::sortbits},
    {"queueheads", one_of(1, 2, 4, 8), "not in {1,2,4,8}", &Options::queueheads, OptionEffect::none},
    {"planregion", zero_or_range(6, 8), "not in {0,6,7,8}", &Options::planregion, OptionEffect::none},
    {"planheavy", in_range(0, 65535), "not in [0, 65535]", &Options::planheavy, OptionEffect::none},
    {"fuse", kOnOff, "not in {0,1}", &Options::fuse, OptionEffect::none},
    {"events", kOnOff, "not in {0,1}", &Options::events, OptionEffect::none},
    {"plistres", zero_or_pow2(16, 4096), "is not 0 or a power of two in [16, 4096]", &Options::plistres, OptionEffect::plistres},
    {"plists", in_range(0, 2), "not in {0,1,2}", &Options::plists, OptionEffect::none},
    {"listres", zero_or_pow2(16, 4096), "is not 0 or a power of two in [16, 4096]", &Options::listres, OptionEffect::listres},
    {"dispatch", in_range(0, 2), "not in {0,1,2}", &Options::dispatch, OptionEffect::none},
    {"ablate", one_of(0, 1, 2, 4, 6, 8, 16, 18, 32, 64), "not in {0,1,2,4,6,8,16,18,32,64}", &Options::ablate, OptionEffect::ablate},
    {"surfaceitems", in_range(0, 1 << 20), "not in [0, 2^20]", &Options::surfaceitems, OptionEffect::none},
    {"skipempty", kOnOff, "not in {0,1}", &Options::skipempty, OptionEffect::none},
    {"rowblock", one_of(0, 1, 2, 4), "not in {0,1,2,4}", &Options::rowblock, OptionEffect::none},
    {"rows", kOnOff, "not in {0,1}", &Options::rows, OptionEffect::none},
    {"queue", kOnOff, "not in {0,1}", &Options::queue, OptionEffect::none},
    {"stack0", one_of(8, 12, 16, 20, 24, 32, 48, 64), "not in {8,12,16,20,24,32,48,64}", &Options::stack0, OptionEffect::stack0},
    {"region", in_range(0, 24), "not in [0,24]", &Options::region, OptionEffect::none},
    {"morton", kOnOff, "not in {0,1}", &Options::morton, OptionEffect::none},
};
constexpr int kOptionCount = (int)(sizeof(kOptions) / sizeof(kOptions[0]));
// kOptions is the set of keys of the strcmp chain it replaced, and tests/test_policy.py writes that set out key by key.  Keys added
// since -- the start table of the lists, the passes over a frame's finished grid -- are rows of the same kind in a table of their own.
constexpr OptionRow kLaterOptions[] = {
    {"starttable", in_range(0, 2), "not in {0,1,2}", &Options::starttable, OptionEffect::none},
    {"lateralpad", kOnOff, "not in {0,1}", &Options::lateralpad, OptionEffect::lateralpad},
    {"fillrounds", in_range(0, 64), "not in [0, 64]", &Options::fillrounds, OptionEffect::none},
    {"mdistwalk", kOnOff, "not in {0,1}", &Options::mdistwalk, OptionEffect::none},
    {"morphform", in_range(0, 2), "not in {0,1,2}", &Options::morphform, OptionEffect::none},
    {"thinrounds", in_range(0, 64), "not in [0, 64]", &Options::thinrounds, OptionEffect::none},
    {"georounds", in_range(0, 64), "not in [0, 64]", &Options::georounds, OptionEffect::none},
    {"accessrounds", in_range(0, 64), "not in [0, 64]", &Options::accessrounds, OptionEffect::none},
    {"sightgroup", one_of(0, 1, 2, 4, 8, 16), "not in {0,1,2,4,8,16}", &Options::sightgroup, OptionEffect::none},
    {"thickcull", in_range(0, 3), "not in {0,1,2,3}", &Options::thickcull, OptionEffect::none},
    {"thickstages", kOnOff, "not in {0,1}", &Options::thickstages, OptionEffect::none},
    {"partprune", in_range(0, 3), "not in {0,1,2,3}", &Options::partprune, OptionEffect::none},
    {"partstages", kOnOff, "not in {0,1}", &Options::partstages, OptionEffect::none},
};

inline const OptionRow* find_option(const char* name)
{
    for (const OptionRow& row : kOptions)
        if (!strcmp(name, row.name)) return &row;
    for (const OptionRow& row : kLaterOptions)
        if (!strcmp(name, row.name)) return &row;
    return nullptr;
}
inline bool option_accepts(const OptionRule& r, int64_t v)
{
    if (r.orZero && v == 0) return true;
    switch (r.kind) {
    case OptionRule::range: return v >= r.lo && v <= r.hi;
    case OptionRule::pow2: return v >= r.lo && v <= r.hi && !(v & (v - 1));
    case OptionRule::set:
        for (int i = 0; r.members[i] >= 0; ++i)
            if (r.members[i] == v) return true;
        return false;
    case OptionRule::sortbits: return v >= r.lo && v <= r.hi && ((v & 15) == 0 || ((v & 15) >= 8 && (v & 15) <= 11));
    }
    return false;
}

} // namespace dxv
