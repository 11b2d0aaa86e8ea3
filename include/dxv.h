/*
 * dxv.h -- C-ABI of the MI355X-native DXRVoxelizer hot path (libdxv.so).
 *
 * Plain C: opaque context, plain pointers and sizes, int return codes (0 = ok, message through
 * dxv_last_error).  No HIP, torch or C++ types cross this boundary.  Each entry point names the
 * reference interface it replaces; paths are relative to /root/reference/DXRVoxelizer/.
 *
 * One context drives one GPU (one process per GPU; see INTEGRATION.md for the multi-GPU slab
 * scheme and the cgo/ctypes/C++ bindings a maintainer of the reference would add).
 */
#ifndef DXV_H
#define DXV_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DXV_API __attribute__((visibility("default")))

/* Bumped whenever an entry point changes its signature or a struct of this header its layout; dxv_api_version() returns the
 * value the loaded library was built with -- a binding compares the two before its first call.
 * 7: dxv_update_frame / dxv_render_async / dxv_stream_wait_frame (the ray-cast into a device render target with per-frame constants);
 *    dxv_stats.render_ms is the selected frame's;
 * 6: dxv_prepare_launch / dxv_prepare_launch_interleaved (the work queue of a static scene as Init-time structure), dxv_warmup,
 *    dxv_stats grows plan_prepared / prepare_ms / warmup_ms, options prepared / prepclear, dxv_build_lists_for_grid prepares the grid
 *    it is given;
 * 5: option plan defaults to 2 (every launch builds its queue and clears its grid: nothing carried from launch to launch; the kept
 *    queue is opt-in), options planregion / planheavy / fuse / queueheads;
 * 4: dxv_stats plan fields describe the work queue, options planorder / planregion gone, dxv_debug_plan_check, dxv_trim;
 * 3: dxv_debug_list_check takes a slab (z0, nz). */
#define DXV_API_VERSION 7
DXV_API int dxv_api_version(void);

typedef struct dxv_ctx dxv_ctx;

/* Occupancy rule. */
enum {
    /* The reference's rule: one radial ray from the voxel centre, closest hit,
     * dot(normalize(interpolated vertex normal), rayDir) > 0.12
     * (Content/Shaders/DXRVoxelizer.hlsl:44-53, :58-85, :132-140, :5). */
    DXV_MODE_REFERENCE = 0,
    /* north_star's second mode on the same traversal engine: +X axis ray, watertight hit count,
     * occupancy = count & 1 (no reference counterpart). */
    DXV_MODE_PARITY = 1,
    /* The conservative (26-separating) surface: a voxel is 1 exactly when its closed box overlaps at
     * least one closed triangle -- Akenine-Moller's separating-axis test in float32 with a fixed
     * operation order, the box centred on the voxel centre of the ray rules,
     * half size 1 / grid_dim.  Marks the thin walls and features a centre rule drops. */
    DXV_MODE_SURFACE = 2,
    /* The solid with its shell: DXV_MODE_REFERENCE's grid OR DXV_MODE_SURFACE's, voxel by voxel. */
    DXV_MODE_REFERENCE_SURFACE = 3
    /* Modes 2 and 3 take the same grids and partitions as 0 and 1; the texel image exists in mode 0 only. */
};

/* What dxv_debug_download copies (tests only; layouts in dxrvoxelizer_amd/csrc/dxv_types.h). */
enum {
    DXV_DBG_SORTED_KEYS = 0, /* T x uint64: (morton30 << 32) | triangle index, ascending   */
    DXV_DBG_NODES = 1,       /* max(T-1,1) x 64 B internal nodes                              */
    DXV_DBG_TRI_POS = 2,     /* T x 48 B: 3 x {x,y,z,w}; w of vertex 0 = triangle index bits  */
    DXV_DBG_TRI_NRM = 3,     /* T x 48 B: 3 x {nx,ny,nz,0}                                    */
    DXV_DBG_PARENTS = 4,     /* (T-1) internal + T leaf parent words: (parent << 1) | side    */
    DXV_DBG_NODES32 = 5,     /* max(T-1,1) x 32 B traversal nodes (half-float boxes)          */
    DXV_DBG_NODES64 = 6,     /* max(T-1,1) x 64 B wide traversal nodes (up to 4 boxes each)   */
    DXV_DBG_LIST_CELLS = 7,  /* 6 R R x 16 B: begin, end, far radius of every texel's list       */
    DXV_DBG_LIST_ENTRIES = 8,/* stats.list_entries x 16 B entries of the direction-space lists  */
    DXV_DBG_LIST_MIP = 9,    /* max-mip of the texels' far radii: 16-bit words, levels R^2 .. 1 x 6 faces */
    /* The display pass's empty-brick flags of the selected frame's last render with option skipempty = 1, M = ceil(grid_dim / 8):
     * refused when the frame has not been rendered with flags, or was launched at another grid size since. */
    DXV_DBG_BRICK_EMPTY = 10,  /* M^3 bytes [bz][by][bx]: 1 where voxels [8b, 8b+8] per axis (clipped to the grid) are all 0 */
    DXV_DBG_BRICK_SUMMARY = 11 /* M^3 bytes behind them: bit0 any voxel of the brick, bit1 any on its x=0 face, bit2 z=0 face,
                                * bit3 x=0,z=0 edge, bit4 y=0 face, bit5 x=0,y=0 edge, bit6 y=0,z=0 edge, bit7 its corner voxel */
};
/* ... and one selector more, of what is derived from the lists: 6 R R x uint32, the lists' start table, one word per texel (made with
 * the lists, whatever option starttable says).  Named like the enum's members; a macro because the enum is a closed set of twelve. */
#define DXV_DBG_LIST_STARTS 12
/* ... and the lists' start cells, 6 R R x 16 B: every texel's cell of DXV_DBG_LIST_CELLS with its word of the start table in place of the
 * three search hints (bytes 10 .. 13; bytes 14, 15 zero) -- what the kernels that read the table read.  Made with the table. */
#define DXV_DBG_LIST_START_CELLS 13

typedef struct dxv_stats {
    uint32_t num_tris, num_verts, num_nodes, tree_height;
    float bound[4];          /* centre.xyz, half extent (Content/Voxelizer.cpp:52-57)          */
    float upload_ms;         /* dxv_set_mesh H2D                                               */
    float prep_ms, sort_ms, hierarchy_ms, refit_ms, build_ms; /* last dxv_build, HIP events   */
    float voxelize_ms;       /* last dxv_voxelize kernel, HIP events on the ctx stream         */
    uint32_t grid_dim, z0, nz; /* last dxv_voxelize                                            */
    uint32_t stack_entries;  /* LDS traversal stack entries per thread of the last launch      */
    float render_ms;         /* the selected frame's last render (flags + ray-cast), HIP events; of a dxv_render_async: read by the frame's next dxv_sync */
    uint32_t redo_rays;      /* rays of the last launch finished by the deep-stack redo pass       */
    uint32_t row_block;      /* parity rule: rows per side of a wave's block of rows (1, 2 or 4)   */
    float tri_extent;        /* mean triangle box extent along y/z, normalised units               */
    uint32_t list_entries;   /* reference rule: entries of the direction-space lists in use, 0 = tree walk */
    uint32_t list_res;       /* ... texels per cube-map face side                                   */
    float list_ms;           /* ... time of their build (first launch after a build / refit / import) */
    uint32_t plan_bricks;    /* reference rule through a work queue: 4^3-voxel bricks queued as possibly holding a live ray (0 = no queue) */
    uint32_t plan_waves;     /* ... persistent single-wave workgroups the launch ran (what the GPU holds at once)        */
    float plan_ms;           /* ... time of the queue's build on the device, in front of the kernel (launches that built one) */
    uint32_t plan_prepared;  /* 1: the last launch ran a queue PREPARED in Init / by dxv_prepare_launch (plan_bricks = its bricks, plan_waves = the
                                workgroups the hardware dealt out, plan_ms = 0: no queue was built inside the launch)                            */
    float prepare_ms;        /* device time of the context's last dxv_prepare_launch* that built a queue (queue build + its sixteen counts)       */
    float warmup_ms;         /* host time dxv_create spent in the process's one warm-up pass on this device (0: another context paid, or none)  */
} dxv_stats;

/* Create a context on HIP device `device` (Voxelizer::Voxelizer + the device objects that
 * Voxelizer::Init receives from its caller, Content/Voxelizer.cpp:19-42).  Fails when no HIP
 * device is present: there is no CPU fallback.
 * A process's first context on a device sends a four-triangle scene through every step once (about 10 ms): what the runtime sets up
 * lazily -- code object, staging of the first upload, the kernels' first dispatch -- is then paid here and not by the caller's first
 * Init, which it would cost 11 ms instead of 3.3 at 1 M triangles.  Environment DXV_WARMUP=0: no such pass. */
DXV_API int dxv_create(dxv_ctx** out, int device);
/* The warm-up pass on its own (idempotent per process and device; dxv_create calls it unless DXV_WARMUP=0): a host that wants its
 * first dxv_create to be cheap, or wants to time the pass, calls it first.  *ms (may be NULL): host milliseconds it took, 0 when
 * the device was warm already.  dxv_stats.warmup_ms of the context whose dxv_create ran the pass says the same. */
DXV_API int dxv_warmup(int device, float* ms);
DXV_API void dxv_destroy(dxv_ctx* ctx);

/* Last error text of this context ("" when none); with ctx == NULL the last dxv_create error.
 * Mirrors the reference's bool-return convention (XUSG/Core/XUSG.h:12-15) plus a message. */
DXV_API const char* dxv_last_error(const dxv_ctx* ctx);

/* Run all work of this context on an existing hipStream_t (e.g. torch's current stream).  NULL
 * restores the context's own stream.  Replaces the caller-owned command list every reference
 * entry point receives (Content/Voxelizer.h:16-22). */
DXV_API int dxv_set_stream(dxv_ctx* ctx, void* hip_stream);

/* Mesh ingest: replaces XUSG::ObjLoader::Import(file, needNorm=true, needAABB=true)
 * (XUSG/Optional/XUSGObjLoader.cpp:18-40, called at Content/Voxelizer.cpp:46-47).  Output layout
 * is the reference's: vb = numVerts x {float3 pos, float3 nrm} (stride 24), ib = numIndices
 * uint32 (already z-negated / reversed), aabb = {min.xyz, max.xyz}.  Free both with dxv_free. */
DXV_API int dxv_obj_load(const char* path, float** vb, uint32_t* num_verts, uint32_t** ib,
                         uint32_t* num_indices, float aabb[6]);
DXV_API void dxv_free(void* p);

/* Upload vertex/index buffers and derive the normalising bound: replaces createVB/createIB and
 * the bound extraction (Content/Voxelizer.cpp:48-57, :115-138).  The arrays are copied; the
 * caller keeps ownership.  vb: num_verts x 6 floats, ib: 3*num_tris uint32 < num_verts. */
DXV_API int dxv_set_mesh(dxv_ctx* ctx, const float* vb, uint32_t num_verts, const uint32_t* ib,
                         uint32_t num_tris);

/* Build the acceleration structure on the device: replaces Voxelizer::buildAccelerationStructures
 * (BLAS + TLAS with the mesh -> [-1,1]^3 instance transform, Content/Voxelizer.cpp:264-326) with
 * an LBVH: Morton keys -> radix sort -> Karras hierarchy -> bottom-up refit. */
DXV_API int dxv_build(dxv_ctx* ctx);

/* Dynamic meshes ("real-time voxelization", README.md:2): the reference API exposes
 * BuildFlag::ALLOW_UPDATE / PERFORM_UPDATE (XUSG/RayTracing/XUSGRayTracing.h:13-22) but the sample
 * never uses them.  dxv_update_vertices replaces the vertex buffer contents (same vertex count,
 * same index buffer; the normalising bound stays the one of dxv_set_mesh, as the reference's
 * m_bound stays the one of Init) and dxv_refit recomputes the boxes of the existing hierarchy. */
DXV_API int dxv_update_vertices(dxv_ctx* ctx, const float* vb, uint32_t num_verts);
/* The same from a DEVICE buffer (6 floats per vertex, on this context's GPU): the reference's vertex buffer is a GPU
 * resource (createVB, Content/Voxelizer.cpp:115-126), and a mesh animated on the GPU -- skinning, simulation -- never
 * passes through the host.  A device-to-device copy ENQUEUED on the context's stream (dxv_set_stream), nothing else:
 *  - ordering before the copy is the caller's: whatever wrote device_vb must be complete, or ordered before this stream (same
 *    stream, or an event the stream waits on), when the call is made -- a producer kernel still running on another stream
 *    would be read half-written;
 *  - the caller's buffer may be reused as soon as the call returns only if it is written on that same stream, else after
 *    dxv_sync_all;
 *  - positions are not inspected on the host (dxv_set_mesh refuses non-finite ones there): the following dxv_refit counts
 *    triangles with a NaN / Inf vertex while it gathers them and fails if there are any (the hierarchy stays: the next
 *    good update refits again).
 * Neither update waits for launches in flight (they read the scene's triangle records, never the vertex buffer).
 *
 * dxv_refit is the ONE host round trip of a refit-per-frame loop  { dxv_update_vertices_device; dxv_refit;
 * dxv_voxelize_async; }  whose grid is consumed on the GPU:
 *  - launches still in flight that have nothing left to report (reference rule through the lists, parity rule through row
 *    lists) are waited for on the device -- frame 0 shares the context's stream, the other frames' streams through an event --
 *    so the refit's kernels queue up behind a running launch; launches through the tree (whose stack can ask for a redo) are
 *    synchronised on the host first, as every launch was before;
 *  - when the scene had lists (or option lists = 2) their counting pass runs behind the refit's kernels, and the entry total
 *    comes back with the root box in the one synchronisation dxv_refit ends with;
 *  - the next launch builds the lists from that count and is queued behind the build without waiting for it; the one verdict
 *    only the host can act on (a texel with more than 65,535 entries: tree walk) is read when the frame is next
 *    synchronised -- dxv_sync, any dxv_grid_* call, the next dxv_refit -- and a frame launched with lists that fail it is
 *    launched again through the tree there.
 * (frames per second of this loop at 1 M triangles: README.md's table, from the round's evidence run) */
DXV_API int dxv_update_vertices_device(dxv_ctx* ctx, const void* device_vb, uint32_t num_verts);
DXV_API int dxv_refit(dxv_ctx* ctx);

/* Voxelize slices [z0, z0+nz) of a grid_dim^3 grid: replaces Voxelizer::voxelize =
 * DispatchRays(GRID_SIZE, GRID_SIZE*GRID_SIZE, 1) (Content/Voxelizer.cpp:351-369) with grid_dim
 * promoted from the GRID_SIZE macro (:8) to a parameter.  grid_dim must be even (an odd grid has
 * a NaN ray at its centre voxel, hlsl:52).  Output: uint8 {0,1}, id = ((iz-z0)*N + iy)*N + ix
 * (hlsl:64-67), i.e. the alpha channel the only consumer reads (Shaders/PSRayCast.hlsl:108).
 * Synchronous: returns after the kernel has finished and its status word was checked. */
DXV_API int dxv_voxelize(dxv_ctx* ctx, uint32_t grid_dim, int mode, uint32_t z0, uint32_t nz);

/* Same launch without the host synchronisation (for back-to-back timing); pair with dxv_sync,
 * which waits for the stream and reports any deferred kernel error. */
DXV_API int dxv_voxelize_async(dxv_ctx* ctx, uint32_t grid_dim, int mode, uint32_t z0, uint32_t nz);
DXV_API int dxv_sync(dxv_ctx* ctx);

/* Frames in flight: the reference's Voxelizer owns FrameCount = 3 grids and every per-frame call takes a
 * frameIndex (static const uint8_t FrameCount, Content/Voxelizer.h:24; m_grids[FrameCount], :110;
 * Render(pCommandList, frameIndex, ...), :21-22; voxelize(pCommandList, frameIndex), Content/Voxelizer.cpp:351-356),
 * so that the GPU works on one grid while the host still reads another.  dxv_set_frame selects the frame the
 * following dxv_voxelize* / dxv_sync / dxv_grid_* / dxv_texels_download / dxv_render* / dxv_update_frame / dxv_distance* / dxv_fill* / dxv_isosurface* / dxv_octree* / dxv_components* / dxv_get_stats calls refer to
 * (default 0).  Each frame owns its grid, texel image, status words and -- frames 1 and 2 -- an internal stream,
 * so launches of different frames overlap on the GPU; scene, candidate lists and options are shared (an extra frame
 * costs its grid).  Calls that change what the frames read (dxv_set_mesh, dxv_build, dxv_scene_import, dxv_set_stream) first
 * wait for every frame -- dxv_refit too, on the device where it can (see there); dxv_sync_all does only that.
 * dxv_update_vertices does NOT wait: launches read
 * the scene's triangle records, not the vertex buffer, so the next frame's vertices upload (on a stream of the library's own)
 * while the current frame's launch still runs -- dxv_voxelize_async, dxv_update_vertices, dxv_refit (waits for the launch),
 * dxv_voxelize_async, ... is a loop whose PCIe time is hidden. */
#define DXV_FRAME_COUNT 3
DXV_API int dxv_set_frame(dxv_ctx* ctx, uint32_t frame_index);
DXV_API int dxv_sync_all(dxv_ctx* ctx);

/* The work queue of a STATIC scene as Init-time structure.  Which 4^3-voxel bricks of a (grid, partition) can hold a live ray is a
 * pure function of the scene's candidate lists, the grid size and the partition -- exactly like the lists are of the scene -- so it
 * can be built where the reference builds everything its frames trace through: once, in Init (Content/Voxelizer.cpp:73, :264-326),
 * leaving a frame ONE dispatch (:351-369).  dxv_prepare_launch builds that queue now (k_plan_bricks once, then a sort of the queued
 * bricks into direction-major order -- the order the lists they read are laid out in; 0.3 ms at 512^3 with three host round trips
 * for its counts) for slices [z0, z0 + nz) of a grid_dim^3 grid -- _interleaved: for rank's share of the
 * block-cyclic partition -- and keeps it with the context, for all its frames, until the scene or its lists change (dxv_set_mesh,
 * dxv_build, dxv_refit, dxv_scene_import, a rebuild of the lists: all drop it).  Every later dxv_voxelize* of that grid_dim and
 * partition in reference mode is then: the grid cleared (only the bricks nobody runs, by workgroups of the same dispatch) + one
 * workgroup per queued brick dealt out by the hardware.  Every voxel is still written in every launch and nothing a launch reads
 * was left behind by another LAUNCH; what is read was left by Init.  Launches of partitions that were not prepared, of scenes
 * without lists (over the caps: tree walk) and of refitted meshes build their queue themselves as before (option plan = 2).
 * Builds the lists first if the scene has none yet (as dxv_build_lists_for_grid does).  Up to 16 partitions per context (least
 * recently used goes).  Not an error when the scene cannot have lists: nothing is prepared then (dxv_stats.prepare_ms = 0). */
DXV_API int dxv_prepare_launch(dxv_ctx* ctx, uint32_t grid_dim, uint32_t z0, uint32_t nz);
DXV_API int dxv_prepare_launch_interleaved(dxv_ctx* ctx, uint32_t grid_dim, uint32_t rank, uint32_t world, uint32_t zblock);

/* Load-balanced multi-GPU partition: the grid's Z axis is cut into blocks of `zblock` slices dealt
 * round-robin to `world` ranks; this call voxelizes the grid_dim/world slices of `rank` (global
 * slice of local slice lz: (lz / zblock * world + rank) * zblock + lz % zblock, ascending) into a
 * compact grid_dim*grid_dim*(grid_dim/world)-byte grid.  Requires zblock to be a power of two and
 * grid_dim % (zblock*world) == 0.
 * Contiguous slabs (dxv_voxelize with z0/nz) starve the GPUs that own empty space; see DESIGN.md. */
DXV_API int dxv_voxelize_interleaved(dxv_ctx* ctx, uint32_t grid_dim, int mode, uint32_t rank, uint32_t world,
                                     uint32_t zblock);
DXV_API int dxv_voxelize_interleaved_async(dxv_ctx* ctx, uint32_t grid_dim, int mode, uint32_t rank,
                                           uint32_t world, uint32_t zblock);

/* Result access.  The grid stays resident on the device (the reference never reads it back,
 * it is consumed by the ray-cast pass on the GPU); download is for callers that want it.
 * dxv_grid_device_ptr: the selected frame's grid after dxv_sync; the caller may also write through it, now or later
 * (see dxv_grid_device_ptr_ro below for what that costs). */
DXV_API void* dxv_grid_device_ptr(dxv_ctx* ctx);
/* The same pointer for READING only (the consumer of the reference's grid SRV, Content/Voxelizer.cpp:371-399).
 * dxv_grid_device_ptr marks the frame as written to by the caller for as long as that pointer lives (until the grid is
 * reallocated by a larger launch): every later launch into the frame then clears the whole grid first instead of keeping
 * the zeros of its own last launch -- a caller who caches the pointer and writes through it later is safe.  This accessor
 * leaves the frame alone. */
DXV_API const void* dxv_grid_device_ptr_ro(const dxv_ctx* ctx);
DXV_API size_t dxv_grid_bytes(const dxv_ctx* ctx);
DXV_API int dxv_grid_download(dxv_ctx* ctx, uint8_t* host, size_t bytes);
/* The same grid as one BIT per voxel, packed on the device before it crosses PCIe (8x fewer
 * bytes): voxel 8j+i of the last launch's slab is bit i of byte j, set iff the voxel is solid; a voxel
 * is solid iff its byte is non-zero (the grid as it is when the kernel runs: a caller who wrote through
 * dxv_grid_device_ptr gets the bits of what was written, whatever the bytes).  The bits behind the last
 * voxel are 0.  bytes = dxv_grid_packed_bytes = ceil(dxv_grid_bytes / 8).  What the reference's consumer
 * reads is this one bit (alpha, Shaders/PSRayCast.hlsl:108). */
DXV_API size_t dxv_grid_packed_bytes(const dxv_ctx* ctx);
DXV_API int dxv_grid_download_packed(dxv_ctx* ctx, uint8_t* host, size_t bytes);
/* Number of solid voxels of the selected frame's grid (the last launch's slab), reduced on the device; a voxel is solid iff its byte
 * is non-zero -- the popcount of dxv_grid_download_packed's bits. */
DXV_API int dxv_grid_count(dxv_ctx* ctx, uint64_t* solid);

/* The same grid as the reference's R10G10B10A2_UNORM texels (float4(Normal, 1), hlsl:83-84,
 * Content/Voxelizer.cpp:65): enable before dxv_voxelize to also fill a uint32 texel per voxel
 * (0 where the shader writes nothing).  Reference mode only. */
DXV_API int dxv_enable_texels(dxv_ctx* ctx, int enable);
DXV_API int dxv_texels_download(dxv_ctx* ctx, uint32_t* host, size_t bytes);

/* The grid's consumer, for visual A/B against the reference: Voxelizer::UpdateFrame + renderRayCast
 * (Content/Voxelizer.cpp:81-106, :371-399; Shaders/VSScreenQuad.hlsl + PSRayCast.hlsl: 128-step
 * march through the grid's alpha with a 32-step light march).  eye and view_proj (row-major, row
 * vectors: v' = v * M, as DirectXMath stores them) are what the app passes to UpdateFrame
 * (DXRVoxelizer.cpp:249-254); pos_scale = {x, y, z, scale} or NULL for the default {0,0,0,1}.
 * Renders the whole grid of the last dxv_voxelize into width*height R8G8B8A8 texels on the host.
 * Synchronous: waits for the frame's launch first and for the image's copy at the end (dxv_render_async below is the
 * reference's frame loop, which does neither). */
DXV_API int dxv_render(dxv_ctx* ctx, const float eye[3], const float view_proj[16], const float pos_scale[4],
                       uint32_t width, uint32_t height, uint8_t* rgba_host);

/* The reference's frame loop: UpdateFrame(frameIndex, eyePt, viewProj) writes that frame's constants, Render(..., frameIndex,
 * rtv, dsv) is voxelize + renderRayCast into a render target on the GPU, FrameCount frames are in flight and the host never waits
 * for an image (Content/Voxelizer.cpp:81-113, :371-399; Content/Voxelizer.h:24).  All three calls refer to the frame selected
 * by dxv_set_frame.
 *
 * dxv_update_frame -- Voxelizer::UpdateFrame (Content/Voxelizer.cpp:81-106): the selected frame's ray-cast constants, computed
 * now from the scene's bound, pos_scale (NULL = {0,0,0,1}), the camera (as for dxv_render) and the viewport (the width / height
 * the reference's Init receives, 1 .. 16384 each).  Kept by the frame until its next dxv_update_frame.  Fails on a singular
 * view/projection chain; then nothing changes. */
DXV_API int dxv_update_frame(dxv_ctx* ctx, const float eye[3], const float view_proj[16], const float pos_scale[4],
                             uint32_t width, uint32_t height);
/* dxv_render_async -- renderRayCast(frameIndex) into a caller's render target (Content/Voxelizer.cpp:371-399): the selected
 * frame's whole grid ray-cast with that frame's constants into width x height R8G8B8A8 texels at device_rgba, row r at
 * device_rgba + r * row_pitch bytes.  The image equals dxv_render's byte for byte.  ENQUEUED on the frame's stream behind the
 * frame's last launch; returns without waiting.  Errors of the launch come back from dxv_sync.
 *  - The host waits only where the device cannot be trusted (the rule of dxv_refit): when the frame's last launch can still
 *    report something -- a tree walk whose column can run out and be redone, lists whose deferred check failed -- the frame is
 *    synchronised first; otherwise the call only enqueues.  A prepared static scene in the reference rule (the lists, the
 *    default) thus renders a frame with NO host round trip: dxv_voxelize_async + dxv_render_async.
 *  - Checked on the host before anything is enqueued, each an error with a message: the frame has constants; its last launch
 *    was the whole grid (not a slab or a share); row_pitch >= width * 4 and a multiple of 4, device_rgba 4-byte aligned;
 *    device_rgba is device memory of this context's device (host and pinned host memory are refused) and the image lies
 *    inside its allocation.
 *  - Frames share nothing while rendering: each owns its constants, its empty-brick flags (option skipempty; growing them waits
 *    for that frame's stream only) and its render events.
 *  - The render target's own ordering belongs to the caller, as the reference keeps one render target per frame
 *    (m_renderTargets[FrameCount]): whatever else writes or reads device_rgba must be ordered against the frame's stream by the
 *    caller (dxv_stream_wait_frame, or a dxv_sync).  Only width * 4 bytes of each row are written: padding bytes inside the
 *    pitch keep their values.
 *  - Option events = 1 (default): the render is bracketed by the frame's own two events, and dxv_stats.render_ms of the frame
 *    is read at the frame's next dxv_sync. */
DXV_API int dxv_render_async(dxv_ctx* ctx, void* device_rgba, size_t row_pitch);
/* dxv_stream_wait_frame -- the reference's barrier to PIXEL_SHADER_RESOURCE (Content/Voxelizer.cpp:376-378): makes hip_stream
 * (a consumer's stream; NULL = the null stream) wait ON THE DEVICE for everything enqueued on the selected frame so far (its
 * launch, its render).  Synchronises on the host first under the same rule as dxv_render_async. */
DXV_API int dxv_stream_wait_frame(dxv_ctx* ctx, void* hip_stream);

/* The exact signed distance field of the selected frame's grid, computed on the device (no reference counterpart, like the surface
 * modes): what collision and clearance queries, offsetting, sphere tracing and level sets read next to the occupancy byte.  The input
 * is the WHOLE grid of the frame's last launch, any mode; a voxel is solid iff its byte is non-zero.  For voxel p = (ix, iy, iz)
 *     d2(p) = min over voxels q of the same grid with solid(q) != solid(p) of (px-qx)^2 + (py-qy)^2 + (pz-qz)^2     (integers)
 *     s(p)  = -1 if solid(p) else +1
 * One 4-byte element per voxel, same index as the grid (id = (iz*N + iy)*N + ix), in one of two formats.
 * Distances are in voxel units, CENTRE TO CENTRE: a voxel next to the boundary has |d| = 1, none has 0.  A caller who places the
 * boundary half-way between two voxels subtracts 0.5 from the magnitude of DXV_DIST_F32.  d2 <= 3 * 2047^2 < 2^24, so the
 * conversion to float is exact and the correctly rounded square root makes DXV_DIST_F32 as reproducible as the integers. */
enum {
    DXV_DIST_SQ_I32 = 0,     /* int32   s(p) * d2(p);                no q exists (grid all empty / all solid): s(p) * 0x7fffffff */
    DXV_DIST_F32 = 1         /* float32 s(p) * sqrtf((float)d2(p));  no q exists: s(p) * INFINITY                                */
};
/* dxv_distance_async -- ENQUEUED on the frame's stream behind the frame's last launch (and behind a render, if one is there);
 * returns without waiting.  Errors of the launch come back from dxv_sync.
 *  - The host waits only under dxv_render_async's rule: when the frame's last launch can still report something, the frame is
 *    synchronised first; otherwise the call only enqueues.  A prepared static scene gets dxv_voxelize_async + dxv_distance_async
 *    with no host round trip.
 *  - Checked on the host before anything is enqueued, each an error with a message: the format is one of the two; the frame has been
 *    launched; its last launch was the whole grid (a slab's or a share's field would need its neighbours' voxels).
 *  - Field (4 * N^3 bytes) and scratch (6 * N^3 bytes: three separable passes, x by bit scans over packed rows, y and z by exact
 *    lower envelopes of parabolas) belong to the frame: frames compute their fields side by side.  dxv_trim gives the scratch back.
 *  - What the field describes is the grid as it is when the kernels run: a caller who wrote through dxv_grid_device_ptr gets the
 *    field of what was written (ordering against the frame's stream is the caller's).
 *  - Option events = 1 (default): the field is bracketed by the frame's own two events; dxv_distance_ms reads them.
 * dxv_distance -- the same + dxv_sync. */
DXV_API int dxv_distance_async(dxv_ctx* ctx, int format);
DXV_API int dxv_distance(dxv_ctx* ctx, int format);
/* The selected frame's field on the device (valid after dxv_sync or on the frame's stream; dxv_stream_wait_frame orders a consumer's
 * stream behind it) and its size, 4 * N^3.  NULL / 0 before the frame's first field.  A field is STALE once its frame is launched
 * again: the pointer, the size and the download then fail (NULL, 0, 1; message through dxv_last_error) rather than hand out the
 * field of a grid that is gone. */
DXV_API const void* dxv_distance_device_ptr(const dxv_ctx* ctx);
DXV_API size_t dxv_distance_bytes(const dxv_ctx* ctx);
/* Copy the field to the host (bytes must be dxv_distance_bytes); synchronises the frame first. */
DXV_API int dxv_distance_download(dxv_ctx* ctx, void* host, size_t bytes);
/* Device time of the selected frame's last field in milliseconds (its three kernels, HIP events), read at the frame's dxv_sync:
 * 0 before that, and under option events = 0.  (A getter of its own: dxv_stats keeps its layout.) */
DXV_API int dxv_distance_ms(dxv_ctx* ctx, float* ms);

/* Exterior flood fill: a robust solid from any grid (no reference counterpart; what binvox does by default).  The ray rules trust the mesh --
 * its normals (mode 0), its being watertight (mode 1); the conservative surface (mode 2) trusts neither, and this pass turns it into a
 * solid: mark what the surface touches, flood the empty space from the border of the grid, call everything the flood cannot reach solid.
 * The same pass closes the internal cavities of any grid.  Input: the WHOLE grid of the selected frame's last launch, any mode (bytes a
 * caller wrote through dxv_grid_device_ptr count too).  For voxel p = (ix, iy, iz) of an N^3 grid
 *     wall(p)    iff byte(p) != 0
 *     border(p)  iff any of ix, iy, iz is 0 or N-1
 *     outside    = the smallest set O with: every p with !wall(p) and border(p) is in O;
 *                  if p in O, q is one of p's 6 face neighbours inside the grid and !wall(q), then q in O
 * Free voxels that touch only along an edge or a corner are NOT connected: the conservative surface separates 26-connected paths, so a
 * 6-connected flood cannot leak through it.  "Reachable from the border" is a set, so the result is unique: the device's grid equals a
 * restatement byte for byte.  An all-zero grid stays all zero; an all-wall grid becomes all 1 (SOLID) or all 0 (INTERIOR). */
enum {
    DXV_FILL_SOLID = 0,      /* byte'(p) = 1 if !outside(p) else 0:              the walls and everything they enclose */
    DXV_FILL_INTERIOR = 1    /* byte'(p) = 1 if !outside(p) && !wall(p) else 0:  the enclosed voxels alone             */
};
/* dxv_fill_async -- the result REPLACES the frame's grid in place, bytes exactly 0 or 1: dxv_grid_*, dxv_grid_count, the packed download,
 * dxv_render* and dxv_distance* then work on the filled grid.  ENQUEUED on the frame's stream behind its launch (render, field); returns
 * without waiting.
 *  - The host waits only under dxv_render_async's rule: when the frame's last launch can still report something, the frame is
 *    synchronised first; otherwise the call only enqueues.
 *  - Checked on the host before anything is enqueued, each an error with a message: `what` is one of the two; the frame has been
 *    launched; its last launch was the whole grid (a slab's or a share's flood would need its neighbours' voxels).
 *  - A flood has no bound on its rounds that is both safe and cheap.  The call enqueues ONE batch of rounds (option fillrounds) and the
 *    write-back; a round returns at once when the round before it changed nothing; whether the batch reached the fixed point is one
 *    page-locked word that is read where the frame is next synchronised, and that synchronisation enqueues further batches from the bit
 *    masks kept in the frame's scratch until one converges.  After dxv_sync the grid is always exact; until then the frame counts as one
 *    that can still report something: dxv_render_async, dxv_distance_async, dxv_stream_wait_frame, dxv_grid_* and a second
 *    dxv_fill_async settle a pending fill first.  The next dxv_voxelize* simply overwrites the grid.
 *  - The scratch (two bit masks, about N^3 / 4 bytes) belongs to the frame: frames fill side by side.  dxv_trim gives it back.
 *  - A distance field made before the fill is stale after it; the texel image is not touched.
 * dxv_fill -- the same + dxv_sync. */
DXV_API int dxv_fill_async(dxv_ctx* ctx, int what);
DXV_API int dxv_fill(dxv_ctx* ctx, int what);
/* The selected frame's last fill as of the frame's last dxv_sync: device time in milliseconds from its first kernel to its last write-back
 * (HIP events, option events = 1; else 0) and the rounds it took, the confirming one included.  Either pointer may be NULL. */
DXV_API int dxv_fill_info(dxv_ctx* ctx, float* ms, uint32_t* rounds);

/* Morphology: the solid of a grid grown or shrunk by the exact Euclidean ball (no reference counterpart).  Offsets and clearance, hollowing
 * (S minus its erosion), opening (spikes thinner than the ball go), closing -- and the remedy where a hole in the mesh wider than a voxel
 * defeats dxv_fill: dilate, fill, erode.  Input: the WHOLE grid of the selected frame's last launch, any mode (bytes a caller wrote through
 * dxv_grid_device_ptr count too); solid(p) iff byte(p) != 0.  radius_sq is an integer r2 and the ball B = { v in Z^3 : vx^2 + vy^2 + vz^2 <= r2 }:
 *     DXV_MORPH_DILATE  out(p) = 1 iff there is q in the grid with solid(q)  and |p - q|^2 <= r2
 *     DXV_MORPH_ERODE   out(p) = 1 iff solid(p) and there is NO q in the grid with !solid(q) and |p - q|^2 <= r2
 *     DXV_MORPH_OPEN    DILATE(ERODE(grid))
 *     DXV_MORPH_CLOSE   ERODE(DILATE(grid))
 * Voxels outside the grid do not exist (dxv_distance's "voxels q of the same grid"): they are not solid for DILATE and not empty for ERODE,
 * so ERODE does not eat a solid where it touches the grid's border and an all-solid grid stays all solid.  With this convention CLOSE is
 * extensive, OPEN anti-extensive and both are idempotent.  Integer geometry: the device's grid equals a restatement byte for byte.  A second,
 * independent statement of the same rule, with d = DXV_DIST_SQ_I32 of the same grid:
 *     DILATE(p) == solid(p) || d(p) <= r2          ERODE(p) == solid(p) && -d(p) > r2 */
enum {
    DXV_MORPH_DILATE = 0,
    DXV_MORPH_ERODE = 1,
    DXV_MORPH_OPEN = 2,
    DXV_MORPH_CLOSE = 3
};
/* dxv_morph_async -- the result REPLACES the frame's grid in place, bytes exactly 0 or 1, like dxv_fill.  ENQUEUED on the frame's stream behind
 * its launch (render, field, fill); returns without waiting.
 *  - The host waits only under dxv_render_async's rule; a pending fill is settled first.
 *  - Checked on the host before anything is enqueued, each an error with a message: op is one of the four; 1 <= radius_sq <= 4096 (the ball
 *    reaches at most 64 voxels along an axis); the frame has been launched; its last launch was the whole grid.
 *  - A fixed number of kernels: no rounds, nothing for a later dxv_sync to settle.  OPEN and CLOSE stay in bit masks between their halves.
 *  - Everything a fill makes stale is stale after a morph: distance field, mesh-distance sign, isosurface, octree, components.  The texel
 *    image is not touched.
 *  - Two forms of the same bytes (option morphform): up to radius_sq 1024 word-parallel on bit masks, whose cost grows with radius_sq; above it
 *    the distance field of the grid and its threshold per half, whose cost does not.
 *  - The scratch (bit masks: 3 + floor(sqrt(radius_sq)) bits per voxel, one more for OPEN and CLOSE; above radius_sq 1024 a field and its
 *    passes, 10 bytes per voxel) belongs to the frame: frames morph side by side.  dxv_trim gives it back.
 * dxv_morph -- the same + dxv_sync. */
DXV_API int dxv_morph_async(dxv_ctx* ctx, int op, uint32_t radius_sq);
DXV_API int dxv_morph(dxv_ctx* ctx, int op, uint32_t radius_sq);
/* The selected frame's last morph as of the frame's last dxv_sync: device time in milliseconds from its first kernel to its write-back (HIP
 * events, option events = 1; else 0), the voxels that became solid and the voxels that became empty.  All 0 before the frame's first morph;
 * any pointer may be NULL. */
DXV_API int dxv_morph_info(dxv_ctx* ctx, float* ms, uint64_t* voxels_set, uint64_t* voxels_cleared);

/* Thinning: the solid of a grid reduced to its skeleton without a change of topology (no reference counterpart).  dxv_morph(ERODE) shrinks a
 * solid but breaks thin parts apart and makes small ones vanish; this operator removes only voxels whose removal changes no piece, cavity or
 * tunnel.  Centre lines of pipes, vessels and limbs; a graph of the shape; with dxv_components and dxv_measure a check of genus.
 * Input: the WHOLE grid of the selected frame's last launch, in any mode.  Bytes written through dxv_grid_device_ptr count too.  solid(p) iff
 * byte(p) != 0.
 * Outside the grid: voxels outside the grid are EMPTY for this operator.  This is UNLIKE dxv_morph, where they do not exist.  The consequence
 * is that an all-solid grid thins from its border.
 * Neighbourhoods of voxel p: N26*(p) is the 26 voxels around p, N18*(p) those of them that share a face or an edge with p, N6*(p) those
 * that share a face.
 * Simple voxel.  Two counts decide it:
 *     T26(p) = the number of 26-connected components of the solid voxels of N26*(p)
 *     T6(p)  = the number of 6-connected components of the EMPTY voxels of N18*(p) that contain a voxel of N6*(p)
 * p is simple iff T26(p) == 1 && T6(p) == 1.  This is the Bertrand-Malandain characterisation for (26, 6) connectivity.  Removing a simple
 * voxel changes no piece, cavity or tunnel.
 * Subfields: sub(p) = (x & 1) | (y & 1) << 1 | (z & 1) << 2 has eight values.  Two distinct voxels of one subfield are never 26-adjacent.
 * One ITERATION, from the current solid set S:
 *     1. B = { p in S : some voxel of N6*(p) is empty }.  This is the border as it is at the START of the iteration.
 *     2. For s = 0, 1, ..., 7 in this order, remove at once from S every p that meets all of: p is in B and still in S; sub(p) == s; p is
 *        simple in the current S; p is not kept by the kind.
 * Whether p is simple depends only on N26*(p), and no other voxel of p's subfield lies in N26*(p): removing a subfield's voxels together
 * equals removing them one by one in any order.  So the result is a function of the grid alone -- it depends on the fixed subfield order and
 * on nothing else (a mirrored grid thins to other bytes) -- and the device's grid equals a restatement byte for byte.
 * Stopping: iterations repeat until one removes nothing -- that iteration is the confirming one, counted like the fill's confirming round
 * -- or until max_iterations of them have run.  max_iterations == 0 means to the fixed point. */
enum {
    DXV_THIN_CURVE = 0,      /* keeps p when exactly one voxel of N26*(p) is solid in the current S, a curve's end point: a curve skeleton */
    DXV_THIN_KERNEL = 1      /* keeps nothing: the topological kernel, one voxel per simply connected piece, a closed one-voxel ring for a torus */
};
/* dxv_thin_async -- the result REPLACES the frame's grid in place, bytes exactly 0 or 1, like dxv_fill and dxv_morph.  ENQUEUED on the frame's
 * stream behind its launch (render, field, fill, morph); returns without waiting.
 *  - The host waits only under dxv_render_async's rule; a pending fill is settled first.
 *  - Checked on the host before anything is enqueued, each an error with a message: the kind is one of the two; the frame has been launched;
 *    its last launch was the whole grid.
 *  - Unbounded iterations by the fill's discipline.  The call enqueues ONE batch of iterations (option thinrounds) and the write-back; an
 *    iteration returns at once when the one before it removed nothing; whether the batch reached the fixed point or max_iterations is a
 *    page-locked block that is read where the frame is next synchronised, and that synchronisation enqueues further batches from the bit masks
 *    kept in the frame's scratch until one confirms.  After dxv_sync the grid is always exact; until then the frame counts as one that can
 *    still report something: dxv_render_async, dxv_distance_async, dxv_fill_async, dxv_morph_async, dxv_components_async, dxv_octree_async,
 *    dxv_isosurface_async, dxv_thickness_async, dxv_geodesic_async, dxv_stream_wait_frame, dxv_grid_* and a second dxv_thin_async settle a pending thin first.  The
 *    next dxv_voxelize* simply overwrites the grid.
 *  - Everything a morph makes stale is stale after a thin: distance field, mesh-distance sign, isosurface, octree, components, thickness.  The texel
 *    image is not touched.
 *  - The scratch (four bit masks, about 3 1/8 bits per voxel) belongs to the frame: frames thin side by side.  dxv_trim gives it back.
 * dxv_thin -- the same + dxv_sync. */
DXV_API int dxv_thin_async(dxv_ctx* ctx, int kind, uint32_t max_iterations);
DXV_API int dxv_thin(dxv_ctx* ctx, int kind, uint32_t max_iterations);
/* The selected frame's last thin as of the frame's last dxv_sync: device time in milliseconds from its first kernel to its last write-back (HIP
 * events, option events = 1; else 0), the iterations it ran, the confirming one included, the voxels it removed, and converged = 0 only when
 * max_iterations stopped it first.  All 0 before the frame's first thin; any pointer may be NULL. */
DXV_API int dxv_thin_info(dxv_ctx* ctx, float* ms, uint32_t* iterations, uint64_t* voxels_removed, int* converged);

/* The exact signed distance from every voxel centre to the MESH, computed on the device by a nearest-triangle query over the scene's
 * hierarchy (no reference counterpart).  dxv_distance above is the field of the GRID -- integer geometry, no |d| below 1, its zero set the
 * staircase of the voxelization; this one is the Euclidean distance to the nearest triangle to sub-voxel accuracy, what collision and
 * clearance queries, offsetting, sphere tracing and level sets want.  Only its SIGN is the grid's: negative where the frame's grid byte
 * is non-zero, so dxv_voxelize + dxv_mesh_distance gives the field of a well-behaved mesh and dxv_voxelize(DXV_MODE_SURFACE) +
 * dxv_fill(DXV_FILL_INTERIOR) + dxv_mesh_distance a robust signed field of a leaky one.
 * For voxel p with centre ((ix+.5)/N*2-1, -((iy+.5)/N*2-1), (iz+.5)/N*2-1) -- the ray rule's -- and the scene's normalised triangles
 *     f(p; a,b,c) = the smallest of the squared distances from p to the nearest point of each edge and to the foot of the perpendicular
 *                   on the face where it lies inside (float32, fixed order: DESIGN.md section 2 writes every operation out)
 *     d2(p)       = min over the triangles of f;  with a band of B > 0 voxels capped at (B * 2/N)^2
 *     tri(p)      = the smallest index (in the caller's index buffer) among the triangles with f == d2(p); 0xffffffff where the cap is
 *                   strictly smaller than every f
 * A minimum does not depend on the order of its terms: the field equals a brute-force restatement bit for bit.  Against the same formula
 * in float64 sqrt(d2) is within 2^-16 normalised units and never more than 2^-20 too small.
 * One float per voxel of the frame's LAST LAUNCH, element ((iz - z0) * N + iy) * N + ix like the grid: the whole grid or a contiguous
 * slab (which needs nothing from its neighbours). */
enum {
    DXV_MDIST_VOXELS_F32 = 0,    /* s(p) * (sqrtf(d2(p)) * (0.5f * N)):  voxel units, like dxv_distance                              */
    DXV_MDIST_UNITS_F32 = 1      /* s(p) * sqrtf(d2(p)):                 normalised units (times bound[3] = object space)            */
};
/* dxv_mesh_distance_async -- ENQUEUED on the frame's stream behind its launch (render, field, fill); returns without waiting.
 *  - The host waits only under dxv_render_async's rule; a pending fill is settled first.  After a dxv_refit that deferred the node boxes
 *    they are brought up to date first, as before a tree walk.
 *  - Checked on the host before anything is enqueued, each an error with a message: the format is one of the two; band_voxels <= 4096
 *    (0: no band); the frame has been launched; its last launch was not an interleaved share; the context has a scene (built or imported).
 *  - want_triangles != 0: tri(p) is stored beside the field (4 more bytes per voxel).
 *  - Field and triangles belong to the frame: frames compute theirs side by side.  dxv_trim keeps them.
 *  - The sign is the grid's as it is when the kernel runs (bytes written through dxv_grid_device_ptr count), the distances are the
 *    scene's as it is then.
 *  - Option events = 1 (default): bracketed by the frame's own two events; dxv_mesh_distance_ms reads them.
 * dxv_mesh_distance -- the same + dxv_sync. */
DXV_API int dxv_mesh_distance_async(dxv_ctx* ctx, int format, uint32_t band_voxels, int want_triangles);
DXV_API int dxv_mesh_distance(dxv_ctx* ctx, int format, uint32_t band_voxels, int want_triangles);
/* The selected frame's field on the device (valid after dxv_sync or on the frame's stream) and its size, 4 bytes per voxel of the launch.
 * NULL / 0 before the frame's first field.  The field is STALE once its frame is launched or filled again: pointer, size and download
 * then fail (NULL, 0, 1; message through dxv_last_error). */
DXV_API const void* dxv_mesh_distance_device_ptr(const dxv_ctx* ctx);
DXV_API size_t dxv_mesh_distance_bytes(const dxv_ctx* ctx);
DXV_API int dxv_mesh_distance_download(dxv_ctx* ctx, void* host, size_t bytes);
/* ... and its nearest triangles, uint32 per voxel (dxv_mesh_distance_bytes as well): NULL / 1 with a message when the field was made
 * without them. */
DXV_API const void* dxv_mesh_distance_triangles_device_ptr(const dxv_ctx* ctx);
DXV_API int dxv_mesh_distance_triangles_download(dxv_ctx* ctx, void* host, size_t bytes);
/* Device time of the selected frame's last mesh distance field in milliseconds (HIP events), read at the frame's dxv_sync: 0 before
 * that, and under option events = 0. */
DXV_API int dxv_mesh_distance_ms(dxv_ctx* ctx, float* ms);

/* Isosurface extraction: a closed triangle mesh from one of the selected frame's signed fields, on the device (no reference counterpart) --
 * the watertight remesh of a leaky model (dxv_voxelize(DXV_MODE_SURFACE) + dxv_fill(DXV_FILL_INTERIOR) + dxv_mesh_distance + dxv_isosurface),
 * an offset surface at iso != 0, a collision proxy at a chosen resolution.  Naive Surface Nets: one vertex in every lattice cell with a sign
 * change, one quad (two triangles) on every lattice edge with one; no case tables, closed and consistently oriented by construction, every
 * arithmetic step fixed (DESIGN.md section 2 writes each out), so the buffers equal a restatement byte for byte.
 *     samples   s(i,j,k) = field[(k*N + j)*N + i] - iso inside the grid; one layer of padding around it is worth +P, one voxel in the field's
 *               unit (1 for the voxel-unit formats, 2 / N for DXV_MDIST_UNITS_F32): a solid that touches the grid's border is capped.
 *               inside(v) iff v < 0 (so -0, +0 and NaN are outside)
 *     vertices  one per cell (cx,cy,cz), each index 0 .. N, whose 8 corners -- the samples c - 1 + (dx,dy,dz) -- are neither all inside nor
 *               all outside: the mean of the linear crossings of the cell's edges (the middle of an edge with a non-finite end), with the
 *               normalised sum of the edges' differences as its normal, pointing out of the solid; ascending cell index
 *               (cz*(N+1) + cy)*(N+1) + cx.  24 bytes {float3 pos, float3 nrm}: an input of dxv_set_mesh as it is
 *     triangles two per crossing lattice edge, over the four cells around it, (b-a) x (c-a) pointing out of the solid in the output space;
 *               uint32 indices; ascending owning cell (the one whose minimum corner is the edge's first sample), then axis x, y, z
 * An all-positive field gives the empty mesh: 0 vertices, 0 triangles, NULL pointers, downloads of 0 bytes -- a success. */
enum {
    DXV_ISO_MESH_DISTANCE = 0,   /* the frame's dxv_mesh_distance field, either format; must be the whole grid's, not a slab's */
    DXV_ISO_GRID_DISTANCE = 1    /* the frame's dxv_distance field in DXV_DIST_F32 (the int32 format is refused)             */
};
enum {
    DXV_ISO_SPACE_VOXELS = 0,    /* voxel index space: coordinate i is the centre of voxel i                                  */
    DXV_ISO_SPACE_OBJECT = 1     /* q = (p + 0.5) / N * 2 - 1 with y and the normal's y negated, then q * bound[3] + bound[0..2]: the mesh's own
                                  * space (needs the scene's bound); every triangle is turned round, because y is mirrored    */
};
/* dxv_isosurface_async -- count and scan kernels ENQUEUED on the frame's stream behind whatever it holds, then ONE host read of two totals
 * (vertices, quads: the mesh's buffers cannot be sized without them), then the emit kernel enqueued; returns without waiting for that.
 *  - The host waits before that only under dxv_render_async's rule; a pending fill is settled first.
 *  - Checked on the host before anything is enqueued, each an error with a message: source and space are known; iso is finite; the frame has
 *    that field and it is not stale; a grid distance field is DXV_DIST_F32; a mesh distance field is the whole grid's; DXV_ISO_SPACE_OBJECT
 *    has a scene to take the bound from.  A mesh of more than 2^31 - 1 vertices or index words is refused once its totals are known.
 *  - Mesh (grow-only vertex and index buffers) and scratch (one bit per lattice cell, two counts per 64 cells) belong to the frame: frames
 *    extract side by side.  dxv_trim gives the scratch back, the mesh stays.
 *  - The mesh is STALE once its frame is launched or filled again: counts, pointers and downloads then fail with a message.
 *  - Option events = 1 (default): bracketed by the frame's own two events; dxv_isosurface_ms reads them at the frame's dxv_sync.
 * dxv_isosurface -- the same + dxv_sync. */
DXV_API int dxv_isosurface_async(dxv_ctx* ctx, int source, float iso, int space);
DXV_API int dxv_isosurface(dxv_ctx* ctx, int source, float iso, int space);
/* Vertices and triangles of the selected frame's mesh (either pointer may be NULL). */
DXV_API int dxv_isosurface_counts(dxv_ctx* ctx, uint32_t* vertices, uint32_t* triangles);
/* The mesh on the device (valid after dxv_sync or on the frame's stream): 24 bytes per vertex, 12 per triangle.  NULL for the empty mesh,
 * and -- with a message -- before the frame's first mesh or when it is stale. */
DXV_API const void* dxv_isosurface_vertices_device_ptr(const dxv_ctx* ctx);
DXV_API const void* dxv_isosurface_indices_device_ptr(const dxv_ctx* ctx);
/* Copies to the host (bytes must be 24 * vertices / 12 * triangles; 0 bytes of the empty mesh are accepted); synchronise the frame first. */
DXV_API int dxv_isosurface_vertices_download(dxv_ctx* ctx, void* host, size_t bytes);
DXV_API int dxv_isosurface_indices_download(dxv_ctx* ctx, void* host, size_t bytes);
/* Device time of the selected frame's last extraction in milliseconds (HIP events; the host's read of the totals lies inside it), read at
 * the frame's dxv_sync: 0 before that, and under option events = 0. */
DXV_API int dxv_isosurface_ms(dxv_ctx* ctx, float* ms);

/* Sparse voxel octree: the selected frame's grid as a tree that is sparse on BOTH sides of the surface, built on the device (no reference
 * counterpart) -- the compact form of a solid for renderers, collision code and storage, and, with dxv_octree_expand, a way to move a grid:
 * build on one context, copy a few megabytes, get the grid back on another.  Every grid can feed it: all four modes, a filled grid, bytes
 * written through dxv_grid_device_ptr.  Every step is fixed, so the node array equals a restatement byte for byte.
 *     input     the WHOLE grid of the frame's last launch, N even, 2 <= N <= 2048; a voxel is solid iff its byte is non-zero
 *     cube      S = the smallest power of two >= N, L = log2 S (1 .. 11); the tree covers [0, S)^3, voxels outside the grid are empty
 *     cells     a cell of level l (0 .. L) has side S >> l; a level-L cell is a voxel, full or empty; a cell above is empty if its eight children
 *               are, full if all eight are full, else mixed; child o = dx | dy << 1 | dz << 2 from the child's position bits
 *     nodes     one for the root and for every mixed cell of levels 1 .. L - 1 (full and empty cells have none), two little-endian uint32:
 *               word1 = mixed (bit o: child o is mixed) | full << 8 (bit o: child o is full), bits 16 - 31 zero; at level L - 1 mixed is 0
 *               word0 = the index of the node of the lowest-numbered mixed child, 0 when mixed is 0; the node of mixed child o is
 *                       word0 + popcount(mixed & ((1 << o) - 1))
 *     order     levels 0, 1, .. L - 1 one after another; inside a level ascending Morton code of the cell position (per bit triple x lowest,
 *               then y, then z): a node's mixed children are consecutive, and the array is unique
 *     table     level_first[0 .. L]: the index of the first node of each level, level_first[L] the total; a level may be empty
 * An all-empty grid is the one node (0, 0x0000), an all-solid 8^3 grid the one node (0, 0xFF00). */
/* dxv_octree_async -- reduce and scan kernels ENQUEUED on the frame's stream behind whatever it holds, then ONE host read of the L + 1 level
 * totals (the node buffer cannot be sized without the last of them), then the emit kernel enqueued; returns without waiting for that.
 *  - The host waits before that only under dxv_render_async's rule; a pending fill is settled first.
 *  - Checked on the host before anything is enqueued, each an error with a message: the frame has been launched; its last launch was the whole
 *    grid, not a slab or a share.  A tree of more than 2^31 - 1 nodes is refused once its totals are known.
 *  - The grid is read once, as it is when the kernels run (bytes written through dxv_grid_device_ptr count).
 *  - Nodes (a grow-only buffer) and scratch belong to the frame: frames build side by side.  The scratch is, for C = 128 + (8^L - 64) / 7 (L >= 2;
 *    64 for L = 1) dense cells of levels 0 .. L - 1 and W = C / 64: 2 C + 8 W + 4 W + 8 ceil(W / 1024) + 96 bytes, each of the five parts rounded up
 *    to 256 -- 0.31 S^3 + 1 KiB, below S^3 / 2 from S = 16 on.  dxv_trim gives it back, the nodes stay.
 *  - The tree is STALE once its frame is launched, filled or expanded again: info, pointer, size and download then fail with a message.
 *  - Option events = 1 (default): bracketed by the frame's own two events; dxv_octree_ms reads them at the frame's dxv_sync.
 * dxv_octree -- the same + dxv_sync. */
DXV_API int dxv_octree_async(dxv_ctx* ctx);
DXV_API int dxv_octree(dxv_ctx* ctx);
/* L, the node count and level_first of the selected frame's tree (any pointer may be NULL; entries of level_first beyond [L] are 0). */
DXV_API int dxv_octree_info(dxv_ctx* ctx, uint32_t* levels, uint32_t* nodes, uint32_t level_first[12]);
/* The nodes on the device (valid after dxv_sync or on the frame's stream), 8 bytes each, and their size.  NULL / 0 -- the pointer with a
 * message -- before the frame's first tree or when it is stale. */
DXV_API const void* dxv_octree_device_ptr(const dxv_ctx* ctx);
DXV_API size_t dxv_octree_bytes(const dxv_ctx* ctx);
/* Copy to the host (bytes must be dxv_octree_bytes); synchronises the frame first. */
DXV_API int dxv_octree_download(dxv_ctx* ctx, void* host, size_t bytes);
/* Device time of the selected frame's last build in milliseconds (HIP events; the host's read of the totals lies inside it), read at the
 * frame's dxv_sync: 0 before that, and under option events = 0. */
DXV_API int dxv_octree_ms(dxv_ctx* ctx, float* ms);
/* dxv_octree_expand_async -- the selected frame's grid FROM an octree, in place: every voxel of the grid becomes a byte of exactly 0 or 1
 * (voxels of the cube beyond the grid are skipped); ENQUEUED on the frame's stream behind whatever it holds, returns without waiting.
 *  - dxv_fill_async's rules: the frame's last launch was the whole grid; the host waits only under dxv_render_async's rule; fields, the mesh and
 *    the frame's own octree made of the grid before are stale after it; the frame's next launch clears its whole grid.
 *  - device_nodes == NULL: the frame's own current tree (`nodes` and `levels` are ignored); stale or none is an error.
 *  - Otherwise a caller's buffer, checked on the host before anything is enqueued, each an error with a message: it is device memory of this
 *    context's device and `nodes` * 8 bytes lie inside its allocation (dxv_render_async's check); it is 4-byte aligned; nodes >= 1; `levels`
 *    equals the L of the frame's grid.
 *  - A caller's buffer is not trusted: every index read from it is compared with `nodes` before it is followed, and a descent stops after L
 *    levels -- never an access outside the buffer.  An index that is refused leaves empty voxels and raises the frame's status: the frame's
 *    next dxv_sync fails with a message, and until then the frame counts as one that can still report something (the next call that
 *    enqueues behind it waits for that verdict first).
 * dxv_octree_expand -- the same + dxv_sync. */
DXV_API int dxv_octree_expand_async(dxv_ctx* ctx, const void* device_nodes, uint32_t nodes, uint32_t levels);
DXV_API int dxv_octree_expand(dxv_ctx* ctx, const void* device_nodes, uint32_t nodes, uint32_t levels);

/* Connected components: what the selected frame's grid CONSISTS of, labelled on the device (no reference counterpart) -- how many separate
 * pieces the solid has, whether a piece is a 40-voxel floater left by a leaky normal, how many closed cavities there are and how big, which
 * voxels to drop so that only the main body is kept: the analysis step between a grid and its field, mesh or tree.  Input: the WHOLE N^3 grid
 * of the selected frame's last launch, as it is when the kernels run (bytes written through dxv_grid_device_ptr count).
 *     member(p)    of = DXV_COMP_SOLID: byte(p) != 0 (dxv_solid.h)      of = DXV_COMP_EMPTY: byte(p) == 0
 *     adjacent     p != q, both inside the grid, |dx|,|dy|,|dz| <= 1, and for connectivity 6: |dx|+|dy|+|dz| == 1; for 26: any
 *     component    a class of the transitive closure of `adjacent` over the members
 *     first(C)     the smallest linear index (iz*N + iy)*N + ix of C's voxels
 *     numbering    components 1 .. K by ascending first(C)
 *     labels[p]    uint32: the number of p's component, 0 when !member(p)
 *     table[k-1]   24 bytes, little endian: uint32 first; uint32 voxels; uint16 lo[3] (x, y, z); uint16 hi[3]; uint32 flags
 *                  flags bit 0: the component has a voxel on the grid's border (any of ix, iy, iz is 0 or N-1); other bits 0
 * Nothing is left to choice, so labels and table are unique: the device's equal a restatement byte for byte.  (The numbering is also the one
 * scipy.ndimage.label gives.) */
enum { DXV_COMP_SOLID = 0, DXV_COMP_EMPTY = 1 };
enum { DXV_SELECT_LARGEST = 0, DXV_SELECT_MIN_VOXELS = 1, DXV_SELECT_BORDER = 2 };
/* dxv_components_async -- pack, union-find and numbering kernels ENQUEUED on the frame's stream behind whatever it holds, then ONE host read
 * of K from a page-locked word (the table cannot be sized without it), then the stats kernels enqueued; returns without waiting for those.
 *  - The host waits before that only under dxv_render_async's rule; a pending fill is settled first.
 *  - Checked on the host before anything is enqueued, each an error with a message: `of` is one of the two kinds; connectivity is 6 or 26; the
 *    frame has been launched; its last launch was the whole grid, not a slab or a share; N <= 1624 (a label and a linear index must both fit a
 *    uint32: 1625^3 < 2^32 < 1626^3, and N is even).
 *  - Labels (N^3 * 4 bytes), table and scratch (two bits per voxel, 4 bytes per 64 voxels, 32 bytes per component) belong to the frame: frames
 *    label side by side.  dxv_trim gives the scratch back and keeps labels and table.
 *  - Labels and table are STALE once the frame is launched, filled, expanded or selected again: info, pointers, sizes and downloads then
 *    fail with a message.
 *  - Option events = 1 (default): bracketed by the frame's own two events; dxv_components_ms reads them at the frame's dxv_sync.
 * dxv_components -- the same + dxv_sync. */
DXV_API int dxv_components_async(dxv_ctx* ctx, int of, int connectivity);
DXV_API int dxv_components(dxv_ctx* ctx, int of, int connectivity);
/* K, the kind and the connectivity of the selected frame's labelling (any pointer may be NULL). */
DXV_API int dxv_components_info(dxv_ctx* ctx, uint32_t* count, int* of, int* connectivity);
/* Labels and table on the device (valid after dxv_sync or on the frame's stream) and their sizes: N^3 * 4 and K * 24 bytes.  NULL / 0 -- the
 * pointers with a message -- before the frame's first labelling or when it is stale; the table's pointer is NULL when K = 0. */
DXV_API const void* dxv_components_labels_device_ptr(const dxv_ctx* ctx);
DXV_API size_t dxv_components_labels_bytes(const dxv_ctx* ctx);
DXV_API const void* dxv_components_table_device_ptr(const dxv_ctx* ctx);
DXV_API size_t dxv_components_table_bytes(const dxv_ctx* ctx);
/* Copies to the host (bytes must be the size above; 0 bytes of an empty table are accepted); synchronise the frame first. */
DXV_API int dxv_components_labels_download(dxv_ctx* ctx, void* host, size_t bytes);
DXV_API int dxv_components_table_download(dxv_ctx* ctx, void* host, size_t bytes);
/* Device time of the selected frame's last labelling in milliseconds (HIP events; the host's read of K lies inside it), read at the frame's
 * dxv_sync: 0 before that, and under option events = 0. */
DXV_API int dxv_components_ms(dxv_ctx* ctx, float* ms);

/* Integral measures: HOW MUCH there is of each component of the selected frame's current labelling, and of all members together -- volume,
 * centre of mass and inertia (from the moments), surface area, and the Euler number, from which the handles and cavities of a solid follow
 * (no reference counterpart).  Input: the labelling as dxv_components left it -- kind `of`, connectivity 6 or 26, K components numbered
 * 1 .. K, label 0 for a non-member.  It must exist and be current: the staleness rule is that of dxv_components_select.  Voxels outside the
 * grid are non-members, as in dxv_components' adjacency.
 * Output: a table of K + 1 records.  Record k (1 .. K) is component k; record 0 is the sum of the others (every measure is additive: every
 * voxel and every cell counted belongs to exactly one component).  K = 0 gives one all-zero record.  A record, 96 bytes, little endian, for
 * component C:
 *     offset  0  uint64    voxels    |C|
 *     offset  8  uint64[3] sum       the sums of ix, iy, iz over C (voxel indices, not centres)
 *     offset 32  uint64[3] sum2      the sums of ix^2, iy^2, iz^2
 *     offset 56  uint64[3] prod      the sums of ix*iy, iy*iz, iz*ix
 *     offset 80  uint64    faces     pairs (p, d): p in C, d one of the six axis steps, p + d a non-member or outside the grid
 *     offset 88  int64     euler     the Euler characteristic of C, by the connectivity of the labelling (so that each cell lies in one component):
 *         connectivity 26   of the complex of closed unit cubes of C: #corners - #edges + #faces - #cubes, a lattice corner, edge or face
 *                           counting iff at least one of the 8, 4 or 2 voxels round it is in C.  (All members round one cell are mutually
 *                           26-adjacent.)  For of = DXV_COMP_SOLID record 0 is the Euler number of the solid, the invariant dxv_thin keeps.
 *         connectivity 6    v - e + f - c: v = |C|, e the 6-adjacent pairs inside C, f the axis-aligned 2 x 2 x 1 squares inside C, c the
 *                           2 x 2 x 2 blocks inside C.  (Every such cell is 6-connected.)
 * A box has euler 1, a hollow box 2, a box with a through tunnel 0, under both.  No sum overflows for N <= 1624, the bound of the labelling:
 * the largest, a sum of ix^2, stays below 1624^5 ~ 1.13e16 < 2^63.  All measures are integers and nothing is left to choice: the device's
 * table equals a restatement byte for byte.
 * dxv_measure_async -- ENQUEUED on the frame's stream behind whatever it holds; returns without waiting and reads nothing back (K is known
 * from the labelling).  One pass over the labelling's member mask; the grid, the labels and the component table are read, never written.
 *  - The host waits only under dxv_render_async's rule; a pending fill or thin is settled first.
 *  - Checked on the host before anything is enqueued, each an error with a message: the frame has been launched (the whole grid); it has a
 *    current labelling.
 *  - The table belongs to the frame: frames measure side by side.  dxv_trim keeps it, as it keeps labels; a measure after dxv_trim packs the
 *    member mask again from the grid.
 *  - The measure is STALE exactly when its labelling is -- the frame was launched, filled, morphed, thinned, expanded or selected again --
 *    and once the frame is labelled again: pointer, size and download then fail with a message.
 *  - Option events = 1 (default): bracketed by the frame's own two events; dxv_measure_ms reads them at the frame's dxv_sync.
 * dxv_measure -- the same + dxv_sync. */
DXV_API int dxv_measure_async(dxv_ctx* ctx);
DXV_API int dxv_measure(dxv_ctx* ctx);
/* The table on the device (valid after dxv_sync or on the frame's stream) and its size, (K + 1) * 96 bytes.  NULL / 0 with a message before
 * the frame's first measure or when it is stale. */
DXV_API const void* dxv_measure_table_device_ptr(const dxv_ctx* ctx);
DXV_API size_t dxv_measure_table_bytes(const dxv_ctx* ctx);
/* Copies it to the host (bytes must be the size above); synchronises the frame first. */
DXV_API int dxv_measure_table_download(dxv_ctx* ctx, void* host, size_t bytes);
/* Device time of the selected frame's last measure in milliseconds (HIP events), read at the frame's dxv_sync: 0 before that, and under
 * option events = 0. */
DXV_API int dxv_measure_ms(dxv_ctx* ctx, float* ms);
/* dxv_components_select_async -- the selected frame's grid edited IN PLACE from its current labels; ENQUEUED on the frame's stream behind
 * whatever it holds, returns without waiting.  A component is kept under
 *     DXV_SELECT_LARGEST     it has the most voxels; ties go to the smaller number.  arg must be 0.
 *     DXV_SELECT_MIN_VOXELS  voxels >= arg
 *     DXV_SELECT_BORDER      flags & 1.  arg must be 0.
 * A voxel of a component that is not kept becomes 0 when of = DXV_COMP_SOLID and 1 when of = DXV_COMP_EMPTY; every other byte stays as it is,
 * values other than 0 and 1 included.  So dxv_components(SOLID) + select(LARGEST) removes floaters; dxv_components(EMPTY) + select(MIN_VOXELS, m)
 * closes cavities and pores below m voxels; after dxv_components(EMPTY, 6) + select(BORDER) the grid's != 0 set is dxv_fill(DXV_FILL_SOLID)'s.
 *  - dxv_fill_async's rules for the grid: the host waits only under dxv_render_async's rule; fields, the mesh and the tree made before are
 *    stale after it, and so are the labels themselves; a kept queue's zeros are dropped: the frame's next launch clears its whole grid.
 *  - Checked on the host before anything is enqueued, each an error with a message: the rule is one of the three; arg is 0 where the rule takes
 *    none; the frame has labels and they are not stale.
 * dxv_components_select -- the same + dxv_sync. */
DXV_API int dxv_components_select_async(dxv_ctx* ctx, int rule, uint32_t arg);
DXV_API int dxv_components_select(dxv_ctx* ctx, int rule, uint32_t arg);
/* The selected frame's last select as of the frame's last dxv_sync: components kept and dropped, and the voxels whose component was dropped
 * (any pointer may be NULL). */
DXV_API int dxv_components_select_info(dxv_ctx* ctx, uint32_t* kept, uint32_t* dropped, uint64_t* voxels_changed);

/* Local thickness: how thick is the part HERE (no reference counterpart).  dxv_distance gives a voxel's depth -- a voxel at the surface of a
 * thick slab has depth 1 -- and dxv_morph(OPEN, r2) says whether a voxel lies in a part at least so thick for ONE radius; this operator gives,
 * per voxel, the largest ball inside the part that reaches the voxel: the minimum wall of a part to print or cast, the necks where it would
 * break, the radius along a dxv_thin skeleton, and, taken of the EMPTY space, channel widths and pore sizes.
 * Input: the WHOLE grid of the selected frame's last launch, in any mode.  Bytes written through dxv_grid_device_ptr count too.  solid(p) iff
 * byte(p) != 0.  Only voxels inside the grid exist, as for dxv_distance and dxv_morph.
 * of = DXV_COMP_SOLID (0) or DXV_COMP_EMPTY (1) picks the members M; cap_sq is an integer, 2 <= cap_sq <= 4096.  Integers only:
 *     D2(c) = min over voxels q of the grid, q not in M, of |c - q|^2      for c in M   (dxv_distance's d2; no such q: +infinity)
 *     R(c)  = min(D2(c), cap_sq)                                            the open ball { p : |p - c|^2 < R(c) } lies inside M
 *     W(p)  = max { R(c) : c in M, |p - c|^2 < R(c) }                       for p in M;   W(p) = 0 for p not in M
 * So 1 <= W(p) <= cap_sq on members, and an all-member grid gives cap_sq everywhere.  A second, independent statement of the same rule, with
 * OPEN(r2) the dxv_morph opening of M and OPEN(0) = M:
 *     W(p) = 1 + max { r2 in 0 .. cap_sq - 1 : p in OPEN(r2) }
 * Two things that are NOT true.  Discrete openings are not nested: { W > r2 } contains OPEN(r2) but does not equal it; only
 * { W == cap_sq } == OPEN(cap_sq - 1) is an equality.  And the capped map is not min(uncapped map, cap_sq): the rule above is the definition.
 * Output: one uint32 per voxel, element (iz * N + iy) * N + ix like the grid, 4 N^3 bytes; and a histogram of cap_sq + 1 uint64, bin v the
 * voxels with W == v, bin 0 the voxels that are no members: the thickness (pore size) distribution, its first non-zero bin above 0 the minimum
 * wall.  A set function of the grid: the device's bytes equal a restatement byte for byte, whatever the order of the atomics.
 * In voxels: 2 sqrt(W) - 1 on members (the host mirrors' thickness_voxels).  A slab k voxels thick reads 2 ceil(k / 2) - 1: balls are centred on
 * voxels, so even thicknesses read as the next odd one.
 * dxv_thickness_async -- ENQUEUED on the frame's stream behind whatever it holds; returns without waiting and reads nothing back: a fixed chain
 * of kernels whose counts stay in device memory.  The grid is read and none of the frame's other products is written -- a current distance
 * field stays current and unchanged: the operator makes its fields in its own scratch.
 *  - The host waits only under dxv_render_async's rule; a pending fill or thin is settled first.
 *  - Checked on the host before anything is enqueued, each an error with a message: of is one of the two; 2 <= cap_sq <= 4096; the frame has
 *    been launched; its last launch was the whole grid; grid_dim <= 1024 (a centre's index is kept in 30 bits).
 *  - Map, histogram and scratch (15 bytes per voxel) belong to the frame: frames run side by side.  dxv_trim gives the scratch back.
 *  - Map and histogram are STALE once the frame is launched, filled, morphed, thinned, expanded or selected again: pointer, sizes and
 *    downloads then fail with a message.
 *  - Option events = 1 (default): bracketed by the frame's own events, read at the frame's dxv_sync.
 * dxv_thickness -- the same + dxv_sync. */
DXV_API int dxv_thickness_async(dxv_ctx* ctx, int of, uint32_t cap_sq);
DXV_API int dxv_thickness(dxv_ctx* ctx, int of, uint32_t cap_sq);
/* The map on the device (valid after dxv_sync or on the frame's stream) and its size, 4 * grid_dim^3 bytes.  NULL / 0 (the pointer with a
 * message) before the frame's first thickness or when it is stale. */
DXV_API const void* dxv_thickness_device_ptr(const dxv_ctx* ctx);
DXV_API size_t dxv_thickness_bytes(const dxv_ctx* ctx);
/* Copies it to the host (bytes must be the size above); synchronises the frame first. */
DXV_API int dxv_thickness_download(dxv_ctx* ctx, void* host, size_t bytes);
/* The histogram: (cap_sq + 1) * 8 bytes, and its copy to the host under the same rules. */
DXV_API size_t dxv_thickness_histogram_bytes(const dxv_ctx* ctx);
DXV_API int dxv_thickness_histogram_download(dxv_ctx* ctx, void* host, size_t bytes);
/* The selected frame's last thickness as of the frame's last dxv_sync: device time in milliseconds from its first kernel to its histogram (HIP
 * events, option events = 1; else 0), the centres whose balls were painted voxel by voxel and the work items -- (centre, z slice) pairs -- they
 * made.  All 0 before the frame's first thickness; any pointer may be NULL. */
DXV_API int dxv_thickness_info(dxv_ctx* ctx, float* ms, uint64_t* centres_painted, uint64_t* work_items);
/* ... and, for measurements, under option thickstages = 1 (else all 0): the times of its six stages, each between events of its own -- the grid's field; E, its field and Top; Top's field
 * (the cull); select, scan and compaction; paint; histogram -- with the voxels the paint loaded and compared and the atomic maxima it sent.
 * The latter depends on the order the work items ran in and differs from run to run; the two pointers may be NULL. */
DXV_API int dxv_thickness_stage_info(dxv_ctx* ctx, float ms[6], uint64_t* voxels_tested, uint64_t* atomics_sent);

/* Maximal-ball partition: cut ONE connected piece at its necks (no reference counterpart).  dxv_components sees one component where the user sees
 * a network; dxv_thickness gives the width per voxel.  This operator gives the bodies and what joins them -- of the EMPTY space the pores and the
 * throats between them with each throat's width, of the SOLID the lobes of a part and the necks between them: the step from per-voxel maps to a
 * graph (Silin & Patzek; Dong & Blunt 2009).
 * Input: the WHOLE grid of the selected frame's last launch, in any mode.  Bytes written through dxv_grid_device_ptr count too.  solid(p) iff
 * byte(p) != 0.  Only voxels inside the grid exist: its border is not "outside", as for dxv_thickness and dxv_distance.
 * of = DXV_COMP_SOLID (0) or DXV_COMP_EMPTY (1) picks the members M; cap_sq is an integer, 1 <= cap_sq <= 4096.  Integers only, with
 * index(v) = (z N + y) N + x and dxv_thickness's R:
 *     R(v)      = min(D2(v), cap_sq) for v in M, 0 elsewhere                (D2: dxv_distance's d2; no voxel outside M: +infinity)
 *     u above v   iff R(u) > R(v), or R(u) == R(v) and index(u) < index(v)  a strict total order on the grid's voxels
 *     parent(c) = the highest voxel of the CLOSED ball { u in the grid : |u - c|^2 <= R(c) }     for c in M
 *     root(c)   = where the chain c, parent(c), parent(parent(c)), ... ends (every step goes strictly up the order)
 * One region per root, numbered 1 .. K by ascending index(root); label(v) = the number of root(v) on members, 0 elsewhere.  A face is a pair of
 * members p, q = p + e, e in {+x, +y, +z}; it is an interface face iff label(p) != label(q).  One throat per unordered pair of labels that share
 * at least one interface face, sorted ascending by (a, b), a < b.
 * Output: labels, one uint32 per voxel, element (iz * N + iy) * N + ix like the grid, 4 N^3 bytes.  The table, K records of 32 bytes, little endian:
 *     uint32 root, radius_sq (= R(root)), voxels, throats; uint16 lo[3], hi[3] (x, y, z); uint32 flags
 * flags bit 0: the region has a voxel with a coordinate 0 or N - 1; throats: the throat records that name the region.  The throats, T records of
 * 20 bytes:
 *     uint32 a, b, faces, neck_sq, neck_voxel
 * faces: the pair's interface faces; neck_sq: the maximum over them of min(R(p), R(q)); neck_voxel: the smallest index(p) among the faces that
 * attain it.  Every step is a set function over the order: the device's bytes equal a restatement byte for byte, whatever ran first.
 * Three properties of the rule, to know and not to "fix":
 *  - A region is a family of balls.  It is 26-connected through its balls but need not be a 6-connected set.
 *  - cap_sq bounds the search's reach.  A body thicker than the cap may fall into several regions: choose cap_sq at least the largest radius^2
 *    of interest.
 *  - A tube of constant width is cut into pieces about its diameter long, and a faceted corner of R = 1 can stay a region of one voxel.
 * dxv_partition_async -- ENQUEUED on the frame's stream behind whatever it holds.  The host waits once in the middle, for K and the number of
 * interface faces -- table and sort cannot be sized without them --, and with want_throats != 0 a second time, for T.  The grid is read and none
 * of the frame's other products is written -- a current distance field, thickness map or labelling stays current and unchanged: the operator
 * makes its field in its own scratch.
 *  - want_throats = 0 skips the throats: the same labels and the same table except each record's `throats` word, which is 0 then; the throats'
 *    pointer, size and download then fail with a message.
 *  - The host waits before that only under dxv_render_async's rule; a pending fill or thin is settled first.
 *  - Checked on the host before anything is enqueued, each an error with a message that leaves the frame's earlier partition and everything else
 *    as it was: of is one of the two; 1 <= cap_sq <= 4096; the frame has been launched; its last launch was the whole grid; grid_dim <= 1024.
 *    No count of regions is refused: a pair of labels is sorted as one word of twice the bits of K.
 *  - Labels, table, throats, scratch (22 bytes per voxel) and the work of the sort belong to the frame: frames run side by side.  dxv_trim gives
 *    scratch and work back.
 *  - Labels, table and throats are STALE once the frame is launched, filled, morphed, thinned, expanded or selected again: pointers, sizes and
 *    downloads then fail with a message.
 *  - Option events = 1 (default): bracketed by the frame's own events, read at the frame's dxv_sync.
 * dxv_partition -- the same + dxv_sync. */
DXV_API int dxv_partition_async(dxv_ctx* ctx, int of, uint32_t cap_sq, int want_throats);
DXV_API int dxv_partition(dxv_ctx* ctx, int of, uint32_t cap_sq, int want_throats);
/* The selected frame's last partition as of the frame's last dxv_sync: device time in milliseconds from its first kernel to its last, the two
 * waits included (HIP events, option events = 1; else 0); K, T and the interface faces of the frame's CURRENT partition (0 when none or stale).
 * Any pointer may be NULL. */
DXV_API int dxv_partition_info(dxv_ctx* ctx, float* ms, uint32_t* regions, uint32_t* throats, uint64_t* interface_faces);
/* Labels, table and throats on the device (valid after dxv_sync or on the frame's stream), their sizes -- 4 * grid_dim^3, 32 K and 20 T bytes --
 * and their copies to the host (bytes must be the size; synchronises the frame first).  NULL / 0 (pointer and download with a message) before the
 * frame's first partition or when it is stale; the throats' also for a partition made with want_throats = 0.  With K = 0 (T = 0) the table's
 * (throats') pointer is NULL and its size 0, without a message. */
DXV_API const void* dxv_partition_labels_device_ptr(const dxv_ctx* ctx);
DXV_API size_t dxv_partition_labels_bytes(const dxv_ctx* ctx);
DXV_API int dxv_partition_labels_download(dxv_ctx* ctx, void* host, size_t bytes);
DXV_API const void* dxv_partition_table_device_ptr(const dxv_ctx* ctx);
DXV_API size_t dxv_partition_table_bytes(const dxv_ctx* ctx);
DXV_API int dxv_partition_table_download(dxv_ctx* ctx, void* host, size_t bytes);
DXV_API const void* dxv_partition_throats_device_ptr(const dxv_ctx* ctx);
DXV_API size_t dxv_partition_throats_bytes(const dxv_ctx* ctx);
DXV_API int dxv_partition_throats_download(dxv_ctx* ctx, void* host, size_t bytes);
/* ... and, for measurements, under option partstages = 1 (else all 0): the times of its six stages, each between events of its own -- the grid's
 * field; keys and mips; the parent search; chain walk, counts and numbering; labels, stats and table; throats -- with the mip cells and the voxels
 * the search tested.  The two pointers may be NULL. */
DXV_API int dxv_partition_stage_info(dxv_ctx* ctx, float ms[6], uint64_t* cells_tested, uint64_t* voxels_tested);

/* Skeleton graph: the nodes and branches of a curve skeleton (no reference counterpart).  dxv_thin leaves centre lines as a grid of bytes; this
 * operator gives the graph they draw -- a label per voxel, a table of nodes (ends and junctions, clustered) and a table of branches (the curves
 * between nodes) with each branch's end nodes, voxel count, exact step counts and, optionally, the minimum, maximum and sum of a caller's
 * per-voxel map along it: the step from a per-voxel map to a graph, as dxv_partition is for pores.
 * Input: the WHOLE grid of the selected frame's last launch, in any mode.  Bytes written through dxv_grid_device_ptr count too.  member(p) iff
 * byte(p) != 0.  Voxels outside the grid are non-members, as for dxv_thin.  Adjacency is dxv_components' at connectivity 26.  Integers only, with
 * index(p) = (z N + y) N + x:
 *     deg(p)     = the members among the 26 neighbours of p                       for a member p
 *     curve(p)   iff deg(p) == 2;   node voxel iff deg(p) != 2   (0: isolated, 1: end, >= 3: junction)
 *     node       a 26-connected component of the node voxels;   numbered 1 .. K by ascending smallest index
 *     branch     a 26-connected component of the curve voxels;  numbered 1 .. B by ascending smallest index
 *     step       an unordered pair {p, q} of adjacent members with at least one of them a curve voxel;
 *                it belongs to the branch of its curve voxel(s); its type is |dx|+|dy|+|dz| - 1  (0 face, 1 edge, 2 corner)
 *     attachment a step whose other voxel is a node voxel: it joins the branch to that voxel's node
 * What deg == 2 gives: a branch is a simple path or a simple closed cycle of curve voxels; two curve voxels that are adjacent are always in the
 * same branch; a path has exactly two attachments (a one-voxel path has both of them) and steps = voxels + 1; a cycle has no attachment, at least
 * 3 voxels, and steps = voxels.  The numbering is scipy.ndimage.label's with the full 3x3x3 structure, as for dxv_components.
 * Output: labels, one uint32 per voxel, element (iz * N + iy) * N + ix like the grid, 4 N^3 bytes: 0 for a non-member, k for a voxel of node k,
 * 0x80000000 | b for a voxel of branch b.  The nodes, K records of 32 bytes, little endian:
 *     uint32 first, voxels, degree, flags; uint16 lo[3], hi[3] (x, y, z); uint32 w_max
 * first: the node's smallest index; degree: the attachments that name the node (a branch from a node back to itself counts 2); flags bit 0: a
 * voxel with a coordinate 0 or N - 1, bit 1: a voxel with deg <= 1, bit 2: a voxel with deg >= 3.  The branches, B records of 48 bytes:
 *     uint32 a, b, first, voxels, steps[3], flags; uint32 w_min, w_max; uint64 w_sum
 * a <= b: the nodes of its two attachments; a == b != 0 is a loop at one node, a == b == 0 a closed cycle.  steps[t]: its steps of type t,
 * attachments included.  flags bit 0: closed, bit 1: a curve voxel with a coordinate 0 or N - 1, bit 2: spur.  A tip is a node with voxels == 1
 * and degree == 1; a spur is a branch of which exactly one of a, b is a tip (with both it is a free segment, not a spur).  w_* are taken over the
 * voxels of the node, or over the curve voxels of the branch, of the caller's uint32 map; all 0 without one.  Length and mean radius are host
 * arithmetic: steps[0] + sqrt(2) steps[1] + sqrt(3) steps[2], and w_sum / voxels.  Every step is a set function of the grid: the device's bytes
 * equal a restatement byte for byte, whatever ran first.
 * Two properties of the rule, to know and not to "fix":
 *  - The rule reads any grid, but it is a graph of the shape only for a grid dxv_thin has left.  A voxel dxv_thin would remove reads as a node or
 *    as a one-voxel loop: the corner voxel of an axis-aligned right angle, whose two neighbours touch each other diagonally, is one.  A square
 *    ring drawn by hand gives 4 nodes of 2 voxels and 4 such loops beside its 4 sides; dxv_thin(DXV_THIN_CURVE) first gives one closed branch.
 *  - A solid blob is one big node.
 * dxv_skeleton_async -- ENQUEUED on the frame's stream behind whatever it holds.  The host waits once in the middle, for K and B -- the tables
 * cannot be sized without them --; then the stats kernels are enqueued.  The grid is read and none of the frame's other products is written -- a
 * current distance field, thickness map or labelling stays current and unchanged.
 *  - device_weights: NULL, or N^3 uint32 on the device laid out like the grid -- another frame's thickness map, for the radius along a branch.
 *    The caller orders whatever wrote it in front of the frame's stream.
 *  - The host waits before that only under dxv_render_async's rule; a pending fill or thin is settled first.
 *  - Checked on the host before anything is enqueued, each an error with a message that leaves the frame's earlier skeleton and everything else
 *    as it was: the frame has been launched; its last launch was the whole grid; grid_dim <= 1024 (bit 31 of a label is the kind);
 *    device_weights is NULL or 4-byte aligned device memory of this context's device with 4 N^3 bytes inside its allocation.
 *  - Labels, tables and scratch (5 bytes per voxel beside the labels) belong to the frame: frames run side by side.  dxv_trim gives the scratch
 *    back and keeps labels and tables.
 *  - Labels and tables are STALE once the frame is launched, filled, morphed, thinned, expanded, selected or pruned again: pointers, sizes and
 *    downloads then fail with a message.
 *  - Option events = 1 (default): bracketed by the frame's own events, read at the frame's dxv_sync.
 * dxv_skeleton -- the same + dxv_sync. */
DXV_API int dxv_skeleton_async(dxv_ctx* ctx, const void* device_weights);
DXV_API int dxv_skeleton(dxv_ctx* ctx, const void* device_weights);
/* The selected frame's last skeleton as of the frame's last dxv_sync: device time in milliseconds from its first kernel to its last, the wait
 * included (HIP events, option events = 1; else 0); K, B and the members with deg <= 1, deg == 2 and deg >= 3 of the frame's CURRENT skeleton (0
 * when none or stale).  Any pointer may be NULL. */
DXV_API int dxv_skeleton_info(dxv_ctx* ctx, float* ms, uint32_t* nodes, uint32_t* branches, uint64_t* end_voxels, uint64_t* curve_voxels, uint64_t* junction_voxels);
/* Labels, nodes and branches on the device (valid after dxv_sync or on the frame's stream), their sizes -- 4 * grid_dim^3, 32 K and 48 B bytes --
 * and their copies to the host (bytes must be the size; synchronises the frame first).  NULL / 0 (pointer and download with a message) before the
 * frame's first skeleton or when it is stale.  With K = 0 (B = 0) the nodes' (branches') pointer is NULL and its size 0, without a message. */
DXV_API const void* dxv_skeleton_labels_device_ptr(const dxv_ctx* ctx);
DXV_API size_t dxv_skeleton_labels_bytes(const dxv_ctx* ctx);
DXV_API int dxv_skeleton_labels_download(dxv_ctx* ctx, void* host, size_t bytes);
DXV_API const void* dxv_skeleton_nodes_device_ptr(const dxv_ctx* ctx);
DXV_API size_t dxv_skeleton_nodes_bytes(const dxv_ctx* ctx);
DXV_API int dxv_skeleton_nodes_download(dxv_ctx* ctx, void* host, size_t bytes);
DXV_API const void* dxv_skeleton_branches_device_ptr(const dxv_ctx* ctx);
DXV_API size_t dxv_skeleton_branches_bytes(const dxv_ctx* ctx);
DXV_API int dxv_skeleton_branches_download(dxv_ctx* ctx, void* host, size_t bytes);
/* dxv_skeleton_prune_async -- removes short spurs from the frame's grid IN PLACE; needs a current skeleton.  For every spur with
 * 3 steps[0] + 4 steps[1] + 5 steps[2] <= max_len345 (dxv_geodesic's chamfer weights, integers) the bytes of the branch's curve voxels and of its
 * tip's one voxel become 0; all such spurs go in one pass, nothing else is touched.  A curve voxel has deg 2 and a tip deg 1, so the removal is a
 * collapse: no piece, tunnel or cavity appears or disappears.  ENQUEUED on the frame's stream under dxv_fill_async's rules for the grid.  It makes
 * stale everything dxv_components_select makes stale, and the skeleton itself.  The recipe:
 *     dxv_thin; dxv_skeleton; dxv_skeleton_prune(L); dxv_thin; dxv_skeleton
 * (the second thin takes what the removal left of a junction).
 * dxv_skeleton_prune -- the same + dxv_sync. */
DXV_API int dxv_skeleton_prune_async(dxv_ctx* ctx, uint32_t max_len345);
DXV_API int dxv_skeleton_prune(dxv_ctx* ctx, uint32_t max_len345);
/* The spurs and the voxels the selected frame's last prune removed, as of the frame's last dxv_sync.  Either pointer may be NULL. */
DXV_API int dxv_skeleton_prune_info(dxv_ctx* ctx, uint32_t* branches_removed, uint64_t* voxels_removed);

/* Geodesic distance: how far one place is from another THROUGH the part, or through its empty space (no reference counterpart).  dxv_distance is
 * the straight-line distance to the other kind of voxel and dxv_fill knows only whether the border can be reached; this operator gives, per
 * member voxel, the length of the shortest path of member voxels to the nearest seed: the length of a dxv_thin skeleton branch, the path between
 * two points of a vessel, the tortuosity of a pore space, how deep a cavity lies behind its channel, and with a limit the geodesic dilation of a
 * marker inside a mask.
 * Input: the WHOLE grid of the selected frame's last launch, in any mode.  Bytes written through dxv_grid_device_ptr count too.  solid(p) iff
 * byte(p) != 0.  Only voxels inside the grid exist.
 * of = DXV_COMP_SOLID (0) or DXV_COMP_EMPTY (1) picks the members M.  metric picks the steps:
 *     DXV_GEO_FACES   = 0   the 6 face neighbours, weight 1                            (G counts steps)
 *     DXV_GEO_CHAMFER = 1   the 26 neighbours: weight 3 face, 4 edge, 5 corner         (G / 3 approximates voxels)
 * A step from p to q is allowed iff both are members and q is a neighbour of p under the metric.  An edge or corner step does not ask about the
 * voxels it squeezes between: the adjacency dxv_components uses at connectivity 26.
 * The seed set S is one of three kinds:
 *     DXV_GEO_SEEDS_BORDER = 0   every voxel with a coordinate equal to 0 or N - 1; seeds and seed_count are ignored
 *     DXV_GEO_SEEDS_LIST   = 1   seeds is a HOST array of seed_count uint32 voxel indices (iz * N + iy) * N + ix, copied before the call returns;
 *                                duplicates are allowed, an index >= N^3 is refused
 *     DXV_GEO_SEEDS_MASK   = 2   seeds is a DEVICE pointer to N^3 bytes, a voxel is a seed iff its byte != 0; it is read on the frame's stream: the
 *                                caller keeps it valid and orders its writer before the call; seed_count is ignored
 * For every kind, seeds that are not members are ignored: seeds_used of dxv_geodesic_info counts the others, |S n M|.
 *     G(p) = min over paths p0 in S n M, p1, ..., pk = p of allowed steps, of the sum of their weights      (0 on seeds)
 *     out(p) = DXV_GEO_NONE      (0xFFFFFFFF)  p not in M
 *              DXV_GEO_UNREACHED (0xFFFFFFFE)  p in M and no path exists, or limit != 0 and G(p) > limit
 *              G(p)                            otherwise
 * limit = 0 means no limit; a voxel with G == limit is kept.  Under a limit the kept values still equal the unlimited G, because every prefix of
 * a shortest path is shorter.  A second, independent statement of the same rule, with out_0 the map of limit 0:
 *     out_limit == where(out_0 <= limit, out_0, UNREACHED) on members
 * An empty S n M is not an error: every member reads UNREACHED.
 * Output: one uint32 per voxel, element (iz * N + iy) * N + ix like the grid, 4 N^3 bytes.  With integer weights G is the unique least fixed
 * point of a relaxation: the device's bytes equal a restatement byte for byte, in whatever order its workgroups run.  A tally goes with it, by
 * one deterministic reduction on the device: the seeds used, the members reached, the members unreached, `farthest` = the greatest G written
 * and `farthest_voxel` = the smallest index that holds it (nothing reached: 0 and 0xFFFFFFFF).
 * dxv_geodesic_async -- ENQUEUED on the frame's stream behind whatever it holds; returns without waiting.  The grid is read and none of the
 * frame's other products is written.
 *  - Rounds without a bound that is both safe and cheap, by the fill's discipline.  The call enqueues the map's first words, ONE batch of rounds
 *    (option georounds) and the tally; whether the batch reached the fixed point is read where the frame is next synchronised, and further
 *    batches are enqueued and waited for there until a round finds nothing to do.  After dxv_sync the map is exact; on the frame's stream alone it
 *    is exact only if one batch was enough.  A map that has not settled after N^3 rounds is an error with a message.
 *  - The host waits only under dxv_render_async's rule; a pending fill, thin, expansion or geodesic of the frame is settled first.
 *  - Checked on the host before anything is enqueued, each an error with a message: of, metric and the seed kind are valid; a LIST has a
 *    non-NULL pointer unless its count is 0, and no index is out of range; a MASK pointer is non-NULL and device memory of N^3 bytes; the frame
 *    has been launched; its last launch was the whole grid; wmax (N^3 - 1) < 0xFFFFFFFE with wmax = 1 or 5, so that no path length can collide
 *    with the two codes (CHAMFER: grid_dim <= 950); grid_dim <= 1024 in any case.
 *  - Map and scratch belong to the frame: frames run side by side.  The map is 4 bytes per voxel; the scratch -- a control block, two sets of
 *    live flags and a queue of 8^3 tiles, 6 bytes per tile = 3/256 byte per voxel, the seeds of a list, the words of a path -- goes back with
 *    dxv_trim, the map stays.
 *  - The map is STALE once the frame's grid version moves -- it is launched, filled, morphed, thinned, expanded or selected again: pointer,
 *    size, download, info and path then fail with a message.
 *  - Option events = 1 (default): bracketed by the frame's own events, read at the frame's dxv_sync.
 * dxv_geodesic -- the same + dxv_sync. */
enum { DXV_GEO_FACES = 0, DXV_GEO_CHAMFER = 1 };
enum { DXV_GEO_SEEDS_BORDER = 0, DXV_GEO_SEEDS_LIST = 1, DXV_GEO_SEEDS_MASK = 2 };
#define DXV_GEO_NONE 0xFFFFFFFFu
#define DXV_GEO_UNREACHED 0xFFFFFFFEu
DXV_API int dxv_geodesic_async(dxv_ctx* ctx, int of, int metric, int seeds_kind, const void* seeds, uint32_t seed_count, uint32_t limit);
DXV_API int dxv_geodesic(dxv_ctx* ctx, int of, int metric, int seeds_kind, const void* seeds, uint32_t seed_count, uint32_t limit);
/* The map on the device (exact after dxv_sync) and its size, 4 * grid_dim^3 bytes.  NULL / 0 (the pointer with a message) before the frame's
 * first geodesic or when it is stale. */
DXV_API const void* dxv_geodesic_device_ptr(const dxv_ctx* ctx);
DXV_API size_t dxv_geodesic_bytes(const dxv_ctx* ctx);
/* Copies it to the host (bytes must be the size above); synchronises the frame first. */
DXV_API int dxv_geodesic_download(dxv_ctx* ctx, void* host, size_t bytes);
/* The selected frame's last geodesic as of the frame's last dxv_sync: device time in milliseconds from its first kernel to its last tally (HIP
 * events, option events = 1; else 0), its rounds with the confirming one, and the tally.  `rounds` may differ from run to run: a tile reads its
 * neighbours' words while they are being lowered, and how soon it sees them decides how many rounds are needed -- never what the map holds.
 * Any pointer may be NULL; fails with a message before the frame's first geodesic or when the map is stale. */
DXV_API int dxv_geodesic_info(dxv_ctx* ctx, float* ms, uint32_t* rounds, uint64_t* seeds_used, uint64_t* reached, uint64_t* unreached, uint32_t* farthest, uint32_t* farthest_voxel);
/* ... and, for measurements, what its rounds did (one entry beyond the rule's list; as of the frame's last dxv_sync, under the same rules): the
 * tiles they ran -- the sum over the rounds of the live 8^3 tiles, so tiles_run / rounds is the live tiles per round --, the most live tiles
 * of one round, and the rounds with fewer than 1024 live tiles, which leave most of the device idle.  Like `rounds`, these differ from run to
 * run. */
DXV_API int dxv_geodesic_work_info(dxv_ctx* ctx, uint64_t* tiles_run, uint32_t* most_live_tiles, uint32_t* sparse_rounds);
/* A shortest path of the selected frame's current map from `target` down to a seed, synchronous (the frame is synchronised first).  target must
 * be in range and hold a value below DXV_GEO_UNREACHED, else an error with a message.  The path starts at p0 = target; the next voxel is the
 * FIRST neighbour q of p_k with out(q) + w(q, p_k) == out(p_k), the neighbours taken in order of increasing index -- dz outermost and dx
 * innermost, each over -1, 0, 1 -- and only the metric's neighbours inside the grid tried; it ends at the first voxel with value 0.  At a fixed
 * point such a q always exists; if none is found the call fails with a message.  *length = the number of voxels on the whole path;
 * min(length, capacity) indices are written to host_path; capacity 0 with a NULL buffer asks for the length alone.  The farthest voxel from
 * the farthest voxel is the usual double sweep for a skeleton's length or a pore network's diameter. */
DXV_API int dxv_geodesic_path(dxv_ctx* ctx, uint32_t target, uint32_t* host_path, uint32_t capacity, uint32_t* length);

/* Access radius and intrusion map: what can reach a voxel from outside, and how large may it be (no reference counterpart).  dxv_thickness is
 * not access-limited -- a wide chamber behind a narrow throat reads "wide", although nothing wider than the throat can get in.  This operator
 * gives, per member voxel, the squared radius of the largest voxel-centred ball whose centre can travel from a seed to it without leaving the
 * members, and the largest such ball that covers it: the mercury-intrusion / drainage curve of a porous sample, whether powder or a cleaning
 * tool of a given radius reaches a cavity of a printed part, the percolation radius between two faces.  It replaces the host loop
 * dxv_morph(ERODE, r), dxv_components, dxv_components_select, dxv_morph(DILATE, r) once per radius.
 * Input: the WHOLE grid of the selected frame's last launch, in any mode.  Bytes written through dxv_grid_device_ptr count too.  solid(p) iff
 * byte(p) != 0.  Only voxels inside the grid exist.
 * of = DXV_COMP_SOLID (0) or DXV_COMP_EMPTY (1) picks the members M.  connectivity is 6 or 26, dxv_components' adjacency: an edge or corner
 * step does not ask about the voxels it squeezes between.  2 <= cap_sq <= 4096 (dxv_thickness's range).  The seed set S is one of
 * dxv_geodesic's three kinds -- DXV_GEO_SEEDS_BORDER, a host LIST of indices, a device MASK --, under the same checks and with the same
 * lifetimes; seeds that are not members are ignored: seeds_used of dxv_access_info counts the others, |S n M|.
 *     R(c) = min(D2(c), cap_sq) for c in M, 0 elsewhere                                        (dxv_thickness's R)
 *     A(c) = max over paths s = p0, p1, ..., pk = c of members, p0 in S n M, consecutive voxels adjacent under `connectivity`,
 *            of  min over the path of R(pi)                       (0 when no such path exists, and for c not in M)
 *     I(p) = max { A(c) : c in M, |p - c|^2 < A(c) }             for p in M (0 when the set is empty), 0 for p not in M
 * A is the access map, I the intrusion map: the access-limited counterpart of dxv_thickness's W.  On seeds A = R.  A <= R, and A <= I <= W on
 * reached members.  Zero means "no member, or not reached"; the tally tells the two apart.  {A > 0} is the reached set of dxv_geodesic for the
 * same seeds, 6 with DXV_GEO_FACES and 26 with DXV_GEO_CHAMFER.  With every member a seed, A == R and I == W, histogram included.
 * The cap: A under cap_sq equals min(A under a larger cap, cap_sq).  This holds for A and NOT for I: a ball of the larger cap covers voxels
 * that no ball of the smaller one does, so I under a cap is not the larger cap's I cut off.
 * Second, independent statements of the same rule:
 *     {A >= t} is the union of the components of {R >= t} under `connectivity` that hold a seed s with R(s) >= t
 *     I(p) = 1 + max { r2 in 0 .. cap_sq - 1 : p in DILATE_r2({A >= r2 + 1}) }, with dxv_morph's closed ball and DILATE_0 the identity; 0 when
 *            there is no such r2 -- the erode / keep-connected / dilate loop, stated once
 * Output: the access map, one uint32 per voxel, element (iz * N + iy) * N + ix like the grid, 4 N^3 bytes; with want_intrusion != 0 the
 * intrusion map, of the same shape; one histogram per map of cap_sq + 1 uint64, bin v the voxels with value v; and a tally by one
 * deterministic reduction on the device: the seeds used, the members reached, the members unreached, `widest` = the greatest A and
 * `widest_voxel` = the smallest index that holds it (nothing reached: 0 and 0xFFFFFFFF).  A is the least fixed point of a monotone relaxation
 * from a fixed start and I is a set function of A: the device's bytes equal a restatement byte for byte, in whatever order its workgroups run.
 * dxv_access_async -- ENQUEUED on the frame's stream behind whatever it holds; returns without waiting.  The grid is read and none of the
 * frame's other products is written.
 *  - The call enqueues the radius field, A's first words, ONE batch of rounds (option accessrounds) and the tally; whether the batch reached
 *    the fixed point is read where the frame is next synchronised, further batches are enqueued and waited for there until a round finds
 *    nothing to do, and the synchronisation that sees that round enqueues the intrusion map and the histograms and waits for them.  After
 *    dxv_sync both maps are exact; on the frame's stream alone only A is, and only if one batch was enough -- the intrusion map and the
 *    histograms do not exist before the frame is synchronised.  A map that has not settled after N^3 rounds is an error with a message.
 *  - The host waits only under dxv_render_async's rule; a pending fill, thin, expansion, geodesic or access of the frame is settled first.
 *  - Checked on the host before anything is enqueued, each an error with a message: of, connectivity, cap_sq and the seed kind are valid; a
 *    LIST has a non-NULL pointer unless its count is 0, and no index is out of range; a MASK pointer is non-NULL and device memory of N^3
 *    bytes; the frame has been launched; its last launch was the whole grid; grid_dim is even, 2 .. 1024.
 *  - Maps, histograms and scratch belong to the frame: frames run side by side.  A map is 4 bytes per voxel; the scratch -- the geodesic's
 *    control block, flags and queue, the radius field and its passes (10 bytes per voxel), with the intrusion map a thickness's scratch (15
 *    bytes per voxel), the seeds of a list -- goes back with dxv_trim, maps and histograms stay.
 *  - Maps and histograms are STALE once the frame's grid version moves -- it is launched, filled, morphed, thinned, expanded or selected
 *    again: pointers, sizes, downloads and infos then fail with a message.
 *  - Option events = 1 (default): bracketed by the frame's own events, read at the frame's dxv_sync.
 * dxv_access -- the same + dxv_sync. */
DXV_API int dxv_access_async(dxv_ctx* ctx, int of, int connectivity, uint32_t cap_sq, int seeds_kind, const void* seeds, uint32_t seed_count, int want_intrusion);
DXV_API int dxv_access(dxv_ctx* ctx, int of, int connectivity, uint32_t cap_sq, int seeds_kind, const void* seeds, uint32_t seed_count, int want_intrusion);
/* The access map on the device (exact after dxv_sync) and its size, 4 * grid_dim^3 bytes; its histogram, (cap_sq + 1) * 8 bytes.  NULL / 0
 * (the pointer with a message) before the frame's first access or when it is stale.  The downloads synchronise the frame first; bytes must be
 * the size above. */
DXV_API const void* dxv_access_device_ptr(const dxv_ctx* ctx);
DXV_API size_t dxv_access_bytes(const dxv_ctx* ctx);
DXV_API int dxv_access_download(dxv_ctx* ctx, void* host, size_t bytes);
DXV_API size_t dxv_access_histogram_bytes(const dxv_ctx* ctx);
DXV_API int dxv_access_histogram_download(dxv_ctx* ctx, void* host, size_t bytes);
/* ... and the intrusion map and its histogram, under the same rules; they also fail with a message (sizes: 0) when the frame's last access
 * was made with want_intrusion = 0.  The map exists once the frame has been synchronised. */
DXV_API const void* dxv_intrusion_device_ptr(const dxv_ctx* ctx);
DXV_API size_t dxv_intrusion_bytes(const dxv_ctx* ctx);
DXV_API int dxv_intrusion_download(dxv_ctx* ctx, void* host, size_t bytes);
DXV_API size_t dxv_intrusion_histogram_bytes(const dxv_ctx* ctx);
DXV_API int dxv_intrusion_histogram_download(dxv_ctx* ctx, void* host, size_t bytes);
/* The selected frame's last access as of the frame's last dxv_sync: device time in milliseconds from its field to its last histogram (HIP
 * events, option events = 1; else 0), its rounds with the confirming one, and the tally.  `rounds` may differ from run to run: a tile reads its
 * neighbours' words while they are being raised -- never what the maps hold.  Any pointer may be NULL; fails with a message before the
 * frame's first access or when the map is stale. */
DXV_API int dxv_access_info(dxv_ctx* ctx, float* ms, uint32_t* rounds, uint64_t* seeds_used, uint64_t* reached, uint64_t* unreached, uint32_t* widest, uint32_t* widest_voxel);
/* ... and, for measurements, what its rounds did, as dxv_geodesic_work_info: the live 8^3 tiles summed over the rounds, the most of one round,
 * and the rounds with fewer than 1024 live tiles.  These differ from run to run. */
DXV_API int dxv_access_work_info(dxv_ctx* ctx, uint64_t* tiles_run, uint32_t* most_live_tiles, uint32_t* sparse_rounds);

/* Line-of-sight map: along which of the 26 lattice directions a straight ray from outside the grid reaches a voxel (no reference
 * counterpart).  dxv_access says what a ball can reach by any path; this operator answers the straight-line question: the undercuts of a mould
 * pulled along an axis and the best of the 13 pull axes, the voxels under an overhang as seen from the build plate, the directions a straight
 * tool, a coating or a cleaning jet gets to a voxel from, a part's shadow volume.  dxv_morph(DXV_MORPH_DILATE, r^2) first gives the sight of a
 * straight tool of radius r.
 * Input: the WHOLE grid of the selected frame's last launch, in any mode.  Bytes written through dxv_grid_device_ptr count too.  solid(p) iff
 * byte(p) != 0.  Only voxels inside the grid exist.
 * of = DXV_COMP_SOLID (0) or DXV_COMP_EMPTY (1) picks the members M.
 * The directions are the 26 vectors d = (dx, dy, dz) in {-1, 0, 1}^3 without 0.  Direction d has bit b(d) = (dz + 1) * 9 + (dy + 1) * 3 +
 * (dx + 1) of a uint32: bits 0 .. 26; bit 13, the zero vector, is never set; DXV_SIGHT_ALL = 0x07FFDFFF.  d and -d have bits b and 26 - b.  The
 * 13 AXES are the pairs (d, -d) with b(d) > 13, axis a = b(d) - 14.  `directions` is a non-empty subset of DXV_SIGHT_ALL.
 *     seen(c, d)   c in M and every voxel c - j d, j = 1, 2, ..., that lies inside the grid is in M: a ray that enters the grid travelling in
 *                  direction d reaches c through members only.  A member with c - d outside the grid is seen along d.
 * Equivalently V_d(c) = M(c) and (c - d outside the grid or V_d(c - d)).  Integers and bits only: the device's bytes equal a restatement byte
 * for byte.
 * Output: the map, one uint32 per voxel, element (iz * N + iy) * N + ix like the grid, 4 N^3 bytes: the OR of the bits of the requested
 * directions along which the voxel is seen, 0 on a voxel that is no member; and a tally of 68 uint64, independent of any order:
 *     [0]        members
 *     [1 + b]    seen[27]: the members seen along direction b; 0 for bit 13 and for a direction not asked for
 *     [28 + a]   neither[13]: for an axis both of whose directions were asked for, the members seen along neither -- the undercut volume of a
 *                two-part mould pulled along that axis; 0 for the other axes
 *     [41 + k]   count[27]: the members seen along exactly k of the requested directions; count[0] is the hidden volume
 * dxv_sight_async -- ENQUEUED on the frame's stream behind whatever it holds; returns without waiting.  The grid is read and none of the
 * frame's other products is written.
 *  - A fixed chain of kernels, nothing to settle: after dxv_sync, or on the frame's stream behind the call, the map is exact.  The tally is
 *    the host's once the frame has been synchronised.
 *  - The host waits only under dxv_render_async's rule; a pending fill, thin, expansion, geodesic or access of the frame is settled first.
 *  - Checked on the host before anything is enqueued, each an error with a message: of is valid; directions is not 0 and has neither bit 13
 *    nor a bit from 27 on; the frame has been launched; its last launch was the whole grid; grid_dim is at most 1024 (the launch has
 *    checked that it is even and at least 2).
 *  - Map and scratch belong to the frame: frames run side by side.  The map is 4 bytes per voxel; the scratch -- the member mask and one bit
 *    plane per requested direction, up to 27 bits per voxel -- goes back with dxv_trim, the map stays.
 *  - Map and tally are STALE once the frame's grid version moves -- it is launched, filled, morphed, thinned, expanded, selected or
 *    dxv_sight_fill'ed again: pointer, size, downloads, info and dxv_sight_fill then fail with a message.
 *  - Option events = 1 (default): bracketed by the frame's own events, read at the frame's dxv_sync.
 * dxv_sight -- the same + dxv_sync. */
enum { DXV_SIGHT_ALL = 0x07FFDFFF };
DXV_API int dxv_sight_async(dxv_ctx* ctx, int of, uint32_t directions);
DXV_API int dxv_sight(dxv_ctx* ctx, int of, uint32_t directions);
/* The map on the device (exact after dxv_sync) and its size, 4 * grid_dim^3 bytes.  NULL / 0 (the pointer with a message) before the frame's
 * first map or when it is stale.  The download synchronises the frame first; bytes must be the size above. */
DXV_API const void* dxv_sight_device_ptr(const dxv_ctx* ctx);
DXV_API size_t dxv_sight_bytes(const dxv_ctx* ctx);
DXV_API int dxv_sight_download(dxv_ctx* ctx, void* host, size_t bytes);
/* The tally, 68 uint64 = 544 bytes, under the same rules. */
DXV_API int dxv_sight_tally_download(dxv_ctx* ctx, void* host, size_t bytes);
/* The selected frame's last map as of the frame's last dxv_sync: device time in milliseconds from its pack to its tally (HIP events, option
 * events = 1; else 0), and what it was made with.  Any pointer may be NULL; fails with a message before the frame's first map or when it is
 * stale. */
DXV_API int dxv_sight_info(dxv_ctx* ctx, float* ms, int* of, uint32_t* directions);
/* The edit from the map, in place: every member of the map's kind whose map word shares no bit with `directions` changes kind -- an EMPTY
 * member becomes 1, the byte dxv_fill writes for solid; a SOLID member becomes 0; every other byte stays as it is.  With one axis' two bits
 * this fills the undercuts of that pull axis; with one bit, the support volume of a build direction; with DXV_SIGHT_ALL, the hidden volume.
 * Needs a current map; `directions` is a non-empty subset of the directions the map was made with.  Enqueued like dxv_morph_async, under
 * dxv_fill_async's rules for the grid: the grid version moves, so this map and every other product of the frame are stale afterwards.
 * Afterwards dxv_sight(of, directions) has count[0] == 0: the line behind a member that is seen consists of members seen along the same
 * direction, so none of them was filled.  dxv_sight_fill -- the same + dxv_sync. */
DXV_API int dxv_sight_fill_async(dxv_ctx* ctx, uint32_t directions);
DXV_API int dxv_sight_fill(dxv_ctx* ctx, uint32_t directions);

/* Multi-GPU: the built scene (nodes + triangle data) as one relocatable device blob, so that
 * rank 0 builds once and the host layer broadcasts it (RCCL over xGMI) to the other ranks.
 * export copies the blob into caller-provided DEVICE memory; import adopts a blob from DEVICE
 * memory as if dxv_set_mesh + dxv_build had run here. */
/* STATIC and DYNAMIC scenes -- the two ways through this header:
 *   static   dxv_set_mesh; dxv_build; dxv_build_lists_for_grid;  then dxv_voxelize* per frame.  The reference's case
 *            (Content/Voxelizer.cpp:73: Init builds everything the frames trace through) and what the host mirrors' Init does
 *            (include/dxv_voxelizer.hpp, dxrvoxelizer_amd/voxelizer.py): LBVH and candidate lists exist when Init returns, and
 *            every launch is the same launch -- it builds its work queue, clears its grid and runs (option plan = 2): a scene's
 *            first Voxelize costs what its hundredth costs.
 *   dynamic  dxv_set_mesh; dxv_build;  then per frame dxv_update_vertices(_device); dxv_refit; dxv_voxelize_async.  The lists of
 *            a mesh that is being refitted are built inside each frame's launch, on the coarser map (option lists, listres).
 * A caller who does neither (dxv_build, then dxv_voxelize) is treated as dynamic until the scene is launched a second time without
 * a refit in between: option lists says when the lists are built then.
 *
 * The candidate lists of the reference rule (direction-space lists): dxv_build_lists builds them now.  A
 * scene exported after that carries them as two more sections of the blob, and the importing contexts adopt them instead of
 * building their own. */
DXV_API int dxv_build_lists(dxv_ctx* ctx);
/* ... on the map the launches of a static scene move to (the 512 map for scenes of 20,000 triangles or more, at every grid size):
 * the exporting rank builds that map before dxv_scene_export, so that the importing ranks do not each rebuild it at their second
 * launch.  Lists that cannot be had on the finer map leave the ones there are.  grid_dim != 0 (even, <= 2048): the whole grid of
 * that size is prepared as well (dxv_prepare_launch(ctx, grid_dim, 0, grid_dim)) -- what the host mirrors' Init does with a grid
 * hint; 0: lists only.  Option lists = 0: nothing is built (the caller asked for tree walks). */
DXV_API int dxv_build_lists_for_grid(dxv_ctx* ctx, uint32_t grid_dim);
/* The same for the parity rule's row lists (option plists): built now instead of at the scene's second parity launch; a scene
 * exported after that carries them too (33 + 72 MB at 1 M triangles), and an importing context adopts them. */
DXV_API int dxv_build_parity_lists(dxv_ctx* ctx);
DXV_API size_t dxv_scene_bytes(const dxv_ctx* ctx);
DXV_API int dxv_scene_export(dxv_ctx* ctx, void* device_dst, size_t bytes);
DXV_API int dxv_scene_import(dxv_ctx* ctx, const void* device_src, size_t bytes);
/* Wrapping 64-bit sum of the 8-byte words of a blob in DEVICE memory of this context's GPU: a host that moves blobs between GPUs
 * compares the receivers' sums with the sender's before it imports anything (once per mesh; include/dxv_multi.hpp, slabs.py). */
DXV_API int dxv_scene_checksum(dxv_ctx* ctx, const void* device_blob, size_t bytes, uint64_t* sum);

DXV_API int dxv_get_stats(const dxv_ctx* ctx, dxv_stats* out);

/* Tuning knobs (kernel variant selection etc.); unknown keys fail.  None changes a result.
 *   brick  0..7   voxels per workgroup (default 4 = 4x4x4, one wavefront)
 *   stack  0|8..64  LDS column entries per thread; 0 (default) = adaptive from stack0
 *   stack0 8..64  starting depth of the adaptive column (default 20)
 *   queue  0|1    postponed-leaf walk (default 1)
 *   wide   0|1|2  reference rule over four-box nodes (1) or on wave-uniform visits only (2, default);
 *                 0 = binary nodes only and no four-box scene section
 *   rows   0|1    parity rule: one tree walk per grid row (default 1)
 *   rowblock 0|1|2|4  ... per row (1), per 2 x 2 or 4 x 4 rows; 0 (default) decides by triangle size
 *   refit  0|1|2  box merge of dxv_build and dxv_refit: min/max pyramid over the leaf order (1,
 *                 default), level sweeps (2), one atomic pass (0)
 *   deferboxes 0|1  dxv_refit while lists are wanted (lists != 0, refit = 1): stop at the pyramid -- triangle records and root
 *                 box are current, the node boxes are written when a tree walk, an export or a debug download first needs them
 *                 (1, default: a refit at 1 M triangles 0.14 -> 0.07 ms); 0 = every refit writes them
 *   lists  0|1|2  reference rule through direction-space lists (dxv_dirmap.h) or the tree walk (0).  The
 *                 lists are built from the scene's triangle records (0.59 ms at 1 M triangles): at the second
 *                 launch after a build / refit / import, or at the first when that launch is large enough for
 *                 the build to pay for itself at once -- 2^26 voxels or more and the estimate after the build's
 *                 counting pass says so (1, default: a mesh refitted every frame takes whichever is faster), or
 *                 always at the first (2); scenes whose lists would exceed 256 entries per triangle + 64 M or
 *                 65,535 entries in one texel keep the tree walk (stats.list_entries = 0)
 *   dispatch 0|1|2  a launch through a KEPT work queue (plan = 1, same lists / partition / buffers as the frame's last launch)
 *                 whose sixteen counts a dxv_sync has read since it was built: one workgroup per queued brick dealt out by the
 *                 hardware (1, default; 2: only for partitions of up to 2^25 voxels) instead of persistent waves (0).  A launch that
 *                 builds its queue (every launch under plan = 2) does not know its size and uses the persistent waves.
 *   listres 0|16..4096  texels per cube-map face side of the lists (power of two).  0 = automatic: 128 below 20,000 triangles,
 *                 256 up to 3 M, 512 beyond -- and the 512 map for every scene of 20,000 triangles or more that is presumed
 *                 STATIC: built by dxv_build_lists / lists = 2 on a scene that has not been refitted, or launched a second time
 *                 without a refit in between (one rebuild).  A mesh that is being refitted, and a first launch whose build
 *                 must pay for itself at once, keep the base map.  Deep scenes (over 32 entries per texel) take coarser maps.
 *   plists 0|1|2    parity rule through row lists of the (y, z) plane: 1 (default) from a scene's second parity launch,
 *                 2 from the first, 0 = always walk the tree; plistres 0|16..4096: texels per side of their grid
 *   plan   0|1|2  lists kernel through a work queue: only the 4^3-voxel bricks that can hold a live ray are run (decided per
 *                 brick on the device, in front of the kernel in the same stream: the brick's footprint in direction space and
 *                 its smallest start radius against a max-mip of the lists' far radii; no host round trip).  The kernel that builds
 *                 the queue clears the partition's grid as well (option fuse), deals the bricks to eight queues -- the bricks that
 *                 can look into a list that is long for the scene at the front (planheavy), every XCD running an equal share of
 *                 all eight -- and persistent waves take them from there.
 *                 2 (default): built and cleared on every launch -- NOTHING is carried from launch to launch: a scene's first,
 *                 second and hundredth launch cost the same and write every voxel;
 *                 1: queue and zeros are kept while the frame's next launch is the same one (same lists, partition, buffers) --
 *                 for a caller that voxelizes a static scene into the same frame again and again (the reference's own loop,
 *                 Content/Voxelizer.cpp:108-113): -13 % per launch at 512^3, -25 % on a rank's share at 8 ranks, and the launch
 *                 goes through the hardware's dispatcher (option dispatch);
 *                 0: no queue, brick box around the scene in Morton order
 *   coop   0|1    the lists kernel: when at most two lanes of a wave are still scanning and the first has 24 entries or more ahead, the whole
 *                 wave scans that ray's list, one entry per lane and round (1, default) -- a brick is as long as its longest list, and a
 *                 short launch (a rank's share) cannot end before its longest brick; 0: every lane scans alone
 *   starttable 0|1|2  the lists' start table, one word per texel made with the lists: from a ray's start radius it says how many entries
 *                 at the head of the texel's list end in front of the ray, and the scan begins behind them (1); 0: the scan begins where
 *                 the start search ends, up to 8 entries early; 2 (default): automatic -- 1 where at least a third of the lists'
 *                 non-empty texels hold more than 8 entries (the word is one more load per ray: it pays where it removes whole scan
 *                 rounds from most waves), else 0, and 0 for a launch queued behind a list build nobody has waited for yet.  A launch
 *                 that reads the table runs brick kernels compiled with it, any other the kernels without.  Same grids either way
 *   lateralpad 0|1  the lists' builder: how far a projected triangle is dilated sideways before its texels and cells are listed.  1 (default):
 *                 a whole, well-shaped projected triangle by the bound derived from the triangle test's own rounding (dxv_dirmap.h:
 *                 dm_lateral_pad), everything else by 2^-15; 0: everything by 2^-15.  Read by the next list build: a change drops the
 *                 lists, their start table and start cells and the prepared queues.  Not part of an exported scene.  Same grids either way
 *   listedwaves 0|8..32 the hardware-dispatched lists kernel (prepared and kept queues, no texel image) fits eight waves per SIMD: 32
 *                 single-wave workgroups per CU.  0 (default): all 32 when the grid side is at least 3/4 of the lists' map side (a brick's rays
 *                 fall on neighbouring texels: 512^3 -9 %, 1024^3 -12 % against seven waves), else 28 (256^3 on the 512 map: a brick is spread
 *                 over many texels and the eighth wave costs 7 %); 8 .. 32: held at so many workgroups per CU by LDS the launch does not use
 *   farmap 0|1    launches over the brick box (tree walks -- lists = 0, dynamic first launches, scenes over the lists' caps -- and plan = 0):
 *                 every workgroup makes the queue's brick test itself and a brick none of whose rays can reach a triangle is zeroed and
 *                 left (1, default); the test reads the lists' max-mip or, for a scene without lists, a far-radius map of the triangles'
 *                 own footprints made at the scene's SECOND such launch (0.13 ms at 1 M triangles: a mesh refitted every frame never pays
 *                 it); 0: every brick is walked
 *   prepared 0|1  launches of a partition that dxv_prepare_launch* prepared use its queue (1, default) or build their own (0)
 *   prepclear 0|1|2|3  how a launch through a prepared queue clears its grid: 0 = a clear kernel in front of the brick kernel; 1 / 2 / 3 =
 *                 only the bricks that are not queued, by workgroups in front of / behind / spread evenly between the bricks' in the
 *                 SAME dispatch
 *   planregion 0|6|7|8  log2 of the run of consecutive Morton bricks that goes to one queue (0 = by partition size)
 *   planheavy 0..65535  a brick that can look into a list of more entries than this goes to the front of its queue (0, default: one
 *                 and a half times the scene's mean at the level of a brick's patch of texels; 65535: no brick does)
 *   fuse   0|1    the queue build clears the grid (1, default) or memsets stand in front of it (0)
 *   queuewaves 0..2^20  persistent waves of a launch through the queue (0, default: what the device holds at once -- 7 per SIMD -- or
 *                 five / four sevenths of that for a mesh of 500,000 triangles or more on a grid of at most half / a quarter of its
 *                 lists' map: 256^3 on the 512 map, nothing carried, -13 % for 1 M-triangle meshes)
 *   queueheads 1|2|4|8  heads per queue the persistent waves draw from (default 8)
 *   queuemin 0..4096  persistent waves beyond one per this many bricks of an XCD's share leave before they touch the queue (0,
 *                 default: all stay; a caller's knob from before queuewaves picked its own default on coarse grids)
 *   sortbits 0|8..11 (+16, +32)  diagnostic, process-wide: widest digit of the builds' radix sort (0, default: 10 or 11 bits -- three
 *                 passes for the LBVH's keys, four for the lists'); +16 / +32: tiles of 4 / 16 waves whatever the size.  Same results.
 *   events 0|1    bracket every launch and every dxv_render_async with two HIP events for stats.voxelize_ms / render_ms (default 1);
 *                 0 for a caller that times its own loop of back-to-back launches (the events cost ~8 us of stream time per launch)
 *   skipempty 0|1 dxv_render, dxv_render_async: skip the samples of empty 8^3 bricks (default 1; same image)
 *   surfaceitems 0..2^20  test hook of the surface modes: work items the large triangles' list may take (0, default: all 2^20 it
 *                 holds); a triangle whose items do not all fit is walked whole as well.  Same grids.
 *   fillrounds 0..64  dxv_fill*: rounds of one batch (0, default: 4 -- the meshes measured take 2 or 3); a fill that needs more is continued
 *                 where its frame is next synchronised.  Same grids.
 *   thinrounds 0..64  dxv_thin*: iterations of one batch (0, default: 16); a thin that needs more is continued where its frame is next
 *                 synchronised.  Same grids.
 *   georounds 0..64  dxv_geodesic*: rounds of one batch (0, default: 16); a geodesic that needs more is continued where its frame is next
 *                 synchronised.  Same map.
 *   accessrounds 0..64  dxv_access*: rounds of one batch (0, default: 16); an access that needs more is continued where its frame is next
 *                 synchronised.  Same maps.
 *   sightgroup 0|1|2|4|8|16  dxv_sight*: lanes of a row group of the sweep at the least; 0 (default) = the next power of two >= the row's 64-bit
 *                 words, which is what a larger value is raised to where it is less (test hook: the widest group without a 514^3 grid).
 *                 Same map, same tally.
 *   morphform 0..2  dxv_morph*: 0 (default) = by the radius: bit planes up to radius_sq 1024, above it the distance field of the grid and its
 *                 threshold, per half; 1 / 2 = always the planes / always the field (measurement, cross-check).  Same grids.
 *   thickcull 0..3  dxv_thickness*: which centres are left out of the paint because their ball cannot raise anything: bit 0 = those whose ball
 *                 lies inside the capped part, bit 1 = those whose ball lies inside a 26-neighbour's (3, default: both; 0: every centre with
 *                 2 <= R < cap_sq is painted; measurement, cross-check).  Same map, same histogram.
 *   thickstages 0|1  dxv_thickness*: 1 = every stage stands between events of its own and the paint counts the voxels it tests and the atomics it
 *                 sends, for dxv_thickness_stage_info (measurement: twelve more event records per call); 0 (default): neither.  Same map.
 *   partprune 0..3  dxv_partition*: which mip levels prune the parent search: bit 0 = the maxima over 4^3 bricks, bit 1 = those over 16^3 cells
 *                 (3, default: both; 0: the plain walk over every ball, r^3 per voxel; measurement, cross-check).  Same labels, table, throats.
 *   partstages 0|1  dxv_partition*: 1 = every stage stands between events of its own and the search counts the mip cells and the voxels it
 *                 tests, for dxv_partition_stage_info (measurement: twelve more event records per call); 0 (default): neither.  Same bytes.
 *   mdistwalk 0|1 dxv_mesh_distance*: 1 (default) = nearest-triangle query over the hierarchy; 0 = every triangle for every voxel, the
 *                 on-device cross-check (seconds on large scenes).  Same field.
 *   morton 0|1, region 0..24, subbox 0|1   brick order, bricks per XCD region (log2), partial launch */
DXV_API int dxv_set_option(dxv_ctx* ctx, const char* key, int64_t value);

/* Test hook: the superset claim of the direction-space lists, checked for every voxel of slices [z0, z0 + nz) of a grid_dim^3
 * grid on the device:
 * every triangle the canonical triangle step accepts for a ray (found by an LBVH walk without distance culling) must be
 * selectable from that ray's texel list.  out[0] = accepted (ray, triangle) pairs, out[1] = violations (must be 0),
 * out[2 + 2k], out[3 + 2k] = voxel id and triangle slot of the first 16 violations.  Builds the lists if needed. */
DXV_API int dxv_debug_list_check(dxv_ctx* ctx, uint32_t grid_dim, uint32_t z0, uint32_t nz, uint64_t out[34]);

/* Test hook: the per-triangle class of the normal test (most hits of the reference rule are answered from two bits of the hit
 * triangle's record instead of its interpolated normal) against the predicate itself: for every voxel of
 * slices [z0, z0 + nz) of a grid_dim^3 grid the closest hit is found by the plain LBVH walk, and when its triangle carries a
 * class the canonical predicate (hlsl:137-138) is evaluated and compared.  out[0] = hits on classified triangles, out[1] =
 * disagreements (must be 0), out[2] = all hits, out[3 + 2k], out[4 + 2k] = voxel id and triangle slot of the first 15. */
DXV_API int dxv_debug_class_check(dxv_ctx* ctx, uint32_t grid_dim, uint32_t z0, uint32_t nz, uint64_t out[34]);

/* Test hook: the ray set-up divides with a scale-free sequence that shares the denominator's reciprocal (csrc/dxv_math.h: div_by) where the
 * canonical rules say `/`; for the operands a voxel origin produces the two are the same bits.  Checked here for EVERY voxel origin of
 * every even grid size n_first, n_first + 2, ... n_last (<= 2048): origin, cube-map point, direction, 1 / direction, shear constants, 14
 * words per voxel against IEEE quotients computed beside them.  out[0] = voxels checked, out[1] = voxels with a differing word (must be
 * 0), out[2 + k] = id of the first 6 (of the grid they occurred in).  All grids up to 2048^3: 2.2 x 10^12 voxels, about a minute. */
DXV_API int dxv_debug_division_check(dxv_ctx* ctx, uint32_t n_first, uint32_t n_last, uint64_t out[8]);

/* Test hook: the brick test of the launches over the brick box (tree walks, plan = 0; option farmap): for every 4^3-voxel brick of slices
 * [z0, z0 + nz) the test the kernel makes, and for every voxel of a brick it calls dead a plain LBVH walk.  lists_mip = 0: against
 * the far-radius map of the triangles' own footprints (what a scene without lists uses; made if need be), 1: against the max-mip of
 * the scene's lists.  out[0] = bricks, out[1] = bricks called dead, out[2] = their rays walked, out[3] = rays among them that hit
 * something (must be 0), out[4 + k] = voxel id of the first 8. */
DXV_API int dxv_debug_far_check(dxv_ctx* ctx, uint32_t grid_dim, uint32_t z0, uint32_t nz, int lists_mip, uint64_t out[12]);

/* Test hook: the work queue's claim -- no live ray in a brick that is not queued -- checked exhaustively on the device for the
 * partition of the current frame's last launch (which must have gone through a queue): every voxel makes exactly the first-step
 * decision of the kernel (origin beyond the root box / texel empty / start beyond the texel's far radius -> miss).
 * out[0] = live voxels, out[1] = bricks with a live voxel, out[2] = queued bricks, out[3] = live bricks that are NOT queued (must
 * be 0), out[4] = bricks queued more than once (must be 0), out[5 + k] = brick word (bx | by << 10 | bz << 20) of the first 11. */
DXV_API int dxv_debug_plan_check(dxv_ctx* ctx, uint64_t out[16]);

/* Test hook: the order of the PREPARED queue that the current frame's last launch ran (direction-major, whole map tiles dealt to
 * the eight queues), read back on the device.  out[0] = queued items, out[1] = direction tiles that appear in more than one queue
 * within the queues' own first ceil(items / 8) items (must be 0), out[2] = neighbouring items of one class (heavy / other) of one
 * queue whose (direction tile, start radius) falls (must be 0), out[3] = a wrapping sum over every (queue, item number, brick word):
 * the same for two builds of the same queue. */
DXV_API int dxv_debug_queue_order(dxv_ctx* ctx, uint64_t out[4]);

/* Test hook: the exclusive scan under the grid operators (octree, components, isosurface, thickness, partition; csrc/scan.hip) on the caller's
 * numbers, in place, on the context's stream.  `lanes` (1 or 2) interleaved values per item.
 *   what = 0: host_counts = items x lanes uint32 counts; each becomes the sum of its lane's counts in front of it, modulo 2^32;
 *             totals[0 .. lanes) = the lanes' sums, 64-bit.
 *   what = 1: host_counts = items x lanes uint64 sums, then `lanes` words the totals are written to -- right behind the sums, where thickness and
 *             partition keep them -- and ONE more word that nothing writes: (items + 1) x lanes + 1 words in all; totals[] = the same totals.
 * Another lane count, items = 0 or host_counts = NULL is refused by the scan's own entry points: non-zero, and host_counts is left as it was. */
DXV_API int dxv_debug_scan(dxv_ctx* ctx, int what, uint32_t lanes, void* host_counts, size_t items, uint64_t totals[2]);

/* Give back what the context keeps only to make the next build faster: the list build's scratch (up to 16 GiB per buffer
 * after a 10 M-triangle scene), the LBVH build's scratch when no refit can follow (imported scenes), the memory of prepared queues
 * whose lists are gone, the scratch of the frames' distance fields (the fields stay), of their flood fills, morphs, thins, thickness and geodesic maps and partitions (maps, labels and tables stay), of their isosurfaces (the
 * meshes stay), of their octrees (the nodes stay) and of their connected components (labels and table stay).  Nothing a launch reads. */
DXV_API int dxv_trim(dxv_ctx* ctx);

/* Test hook: copy an internal device array to the host (enum above). */
DXV_API int dxv_debug_download(dxv_ctx* ctx, int what, void* host, size_t bytes);

#ifdef __cplusplus
}
#endif
#endif /* DXV_H */
