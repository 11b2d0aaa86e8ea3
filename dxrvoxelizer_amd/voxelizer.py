"""Python mirror of the reference's Voxelizer component (Content/Voxelizer.h:10-24) over the
C-ABI, used by tests and bench.py.  Same call order as the reference: Init (load, upload, bound,
build acceleration structure) then Voxelize per frame."""
import ctypes as C
import os

import numpy as np

from ._lib import DxvError, Stats, load_library

MODE_REFERENCE, MODE_PARITY = 0, 1
MODE_SURFACE, MODE_REFERENCE_SURFACE = 2, 3      # the conservative surface; the reference rule's solid with that shell (include/dxv.h)
DIST_SQ_I32, DIST_F32 = 0, 1                     # formats of the distance field (include/dxv.h)
MDIST_VOXELS_F32, MDIST_UNITS_F32 = 0, 1          # formats of the mesh distance field (include/dxv.h)
FILL_SOLID, FILL_INTERIOR = 0, 1                  # what the flood fill leaves (include/dxv.h)
MORPH_DILATE, MORPH_ERODE, MORPH_OPEN, MORPH_CLOSE = 0, 1, 2, 3     # the operations of Morph (include/dxv.h)
THIN_CURVE, THIN_KERNEL = 0, 1                                      # the kinds of Thin (include/dxv.h)
ISO_MESH_DISTANCE, ISO_GRID_DISTANCE = 0, 1       # the field an isosurface is taken from (include/dxv.h)
ISO_SPACE_VOXELS, ISO_SPACE_OBJECT = 0, 1         # ... and the space its vertices are in
COMP_SOLID, COMP_EMPTY = 0, 1                     # what connected components are taken of (include/dxv.h)
SIGHT_ALL = 0x07FFDFFF                            # the 26 directions of Sight: bit (dz + 1) * 9 + (dy + 1) * 3 + (dx + 1), never bit 13 (include/dxv.h)
GEO_FACES, GEO_CHAMFER = 0, 1                     # the metrics of Geodesic (include/dxv.h)
GEO_SEEDS_BORDER, GEO_SEEDS_LIST, GEO_SEEDS_MASK = 0, 1, 2
GEO_NONE, GEO_UNREACHED = 0xFFFFFFFF, 0xFFFFFFFE  # ... and the two codes of its map
SELECT_LARGEST, SELECT_MIN_VOXELS, SELECT_BORDER = 0, 1, 2   # which components SelectComponents keeps
COMP_RECORD = np.dtype([("first", "<u4"), ("voxels", "<u4"), ("lo", "<u2", (3,)), ("hi", "<u2", (3,)), ("flags", "<u4")])   # a row of the components' table, 24 bytes
# a row of the measures' table, 96 bytes (include/dxv.h over dxv_measure_async)
MEASURE_RECORD = np.dtype([("voxels", "<u8"), ("sum", "<u8", (3,)), ("sum2", "<u8", (3,)), ("prod", "<u8", (3,)), ("faces", "<u8"), ("euler", "<i8")])
# a row of a partition's table, 32 bytes, and one of its throats, 20 bytes (include/dxv.h over dxv_partition_async)
PART_REGION = np.dtype([("root", "<u4"), ("radius_sq", "<u4"), ("voxels", "<u4"), ("throats", "<u4"), ("lo", "<u2", (3,)), ("hi", "<u2", (3,)), ("flags", "<u4")])
PART_THROAT = np.dtype([("a", "<u4"), ("b", "<u4"), ("faces", "<u4"), ("neck_sq", "<u4"), ("neck_voxel", "<u4")])
# a node and a branch of a skeleton graph, 32 and 48 bytes (include/dxv.h over dxv_skeleton_async)
SKELETON_NODE = np.dtype([("first", "<u4"), ("voxels", "<u4"), ("degree", "<u4"), ("flags", "<u4"), ("lo", "<u2", (3,)), ("hi", "<u2", (3,)), ("w_max", "<u4")])
SKELETON_BRANCH = np.dtype([("a", "<u4"), ("b", "<u4"), ("first", "<u4"), ("voxels", "<u4"), ("steps", "<u4", (3,)), ("flags", "<u4"), ("w_min", "<u4"), ("w_max", "<u4"),
                            ("w_sum", "<u8")])
SKELETON_BRANCH_BIT = 0x80000000                    # labels: 0 no member, k node k, SKELETON_BRANCH_BIT | b branch b
SKELETON_CLOSED, SKELETON_BORDER, SKELETON_SPUR = 1, 2, 4     # flags of a branch
DBG_SORTED_KEYS, DBG_NODES, DBG_TRI_POS, DBG_TRI_NRM, DBG_PARENTS, DBG_NODES32, DBG_NODES64, DBG_LIST_CELLS, DBG_LIST_ENTRIES, DBG_LIST_MIP = range(10)
DBG_BRICK_EMPTY, DBG_BRICK_SUMMARY = 10, 11         # the display pass's empty-brick flags and the summaries behind them
DBG_LIST_STARTS = 12                                # the lists' start table: one word per texel
DBG_LIST_START_CELLS = 13                           # the lists' start cells: the cells with that word in place of the search hints


def obj_load(path):
    """(vb [V,6] f32, ib [3T] u32, aabb [6] f32) exactly as XUSG::ObjLoader::Import(path, true, true)
    (XUSG/Optional/XUSGObjLoader.cpp:18-40) -- the product's own loader (csrc/obj_ingest.cpp)."""
    lib = load_library()
    vb, ib = C.POINTER(C.c_float)(), C.POINTER(C.c_uint32)()
    nv, ni = C.c_uint32(), C.c_uint32()
    aabb = np.zeros(6, np.float32)
    rc = lib.dxv_obj_load(os.fsencode(path), C.byref(vb), C.byref(nv), C.byref(ib), C.byref(ni), aabb)
    if rc:
        raise DxvError(f"dxv_obj_load({path!r}) failed with code {rc}")
    try:
        return (np.ctypeslib.as_array(vb, (nv.value, 6)).copy(), np.ctypeslib.as_array(ib, (ni.value,)).copy(), aabb)
    finally:
        lib.dxv_free(vb)
        lib.dxv_free(ib)


def betti_numbers(pieces, cavities, euler):
    """(b0, b1, b2) from the pieces, the cavities and the Euler number b0 - b1 + b2 of a solid"""
    return int(pieces), int(pieces) + int(cavities) - int(euler), int(cavities)


def mass_properties(table):
    """Mass properties of every record of a measures' table (dtype MEASURE_RECORD), in voxel units and at unit density, as a dict of float64
    arrays over the records: volume [R]; centroid [R, 3], at voxel centres (ix + 1/2); area [R] = faces; inertia [R, 3, 3], the tensor about
    the centroid with each voxel's own cube (1/6 per axis).  The central second moments are formed exactly, in Python integers, before the
    one division: V * sum2 - sum^2 reaches 1e25, and a difference of floats of that size would keep no digit of a small box far from the
    origin.  A record without voxels has a centroid of NaN and zeros elsewhere.  A pure host function."""
    table = np.atleast_1d(np.asarray(table, MEASURE_RECORD))
    R = len(table)
    out = {"volume": np.zeros(R), "centroid": np.full((R, 3), np.nan), "area": np.zeros(R), "inertia": np.zeros((R, 3, 3))}
    for r, rec in enumerate(table):
        V = int(rec["voxels"])
        out["volume"][r], out["area"][r] = V, int(rec["faces"])
        if not V:
            continue
        s, s2, pr = [int(a) for a in rec["sum"]], [int(a) for a in rec["sum2"]], [int(a) for a in rec["prod"]]
        central = [V * s2[a] - s[a] * s[a] for a in range(3)]           # V * sum of (x - mean)^2, exact
        for a in range(3):
            b, c = (a + 1) % 3, (a + 2) % 3
            out["centroid"][r, a] = (2 * s[a] + V) / (2 * V)
            out["inertia"][r, a, a] = (6 * (central[b] + central[c]) + V * V) / (6 * V)
            cross = V * pr[a] - s[a] * s[b]                             # prod[a] pairs axis a with axis a + 1: xy, yz, zx
            out["inertia"][r, a, b] = out["inertia"][r, b, a] = -cross / V
    return out


def pore_network(table, throats):
    """A partition's table and throats (PartitionTable, PartitionThroats) as a network, in voxels: {"radius": float64 [K], sqrt(radius_sq) of every
    region's largest ball; "voxels": int64 [K]; "coordination": int64 [K], the throats that name the region; "pairs": int64 [T, 2], the labels a < b
    of every throat; "neck_radius": float64 [T], sqrt(neck_sq); "faces": int64 [T]}.  Labels count from 1: region k is row k - 1.  Pure numpy."""
    table, throats = np.atleast_1d(np.asarray(table, PART_REGION)), np.atleast_1d(np.asarray(throats, PART_THROAT))
    return {"radius": np.sqrt(table["radius_sq"].astype(np.float64)), "voxels": table["voxels"].astype(np.int64), "coordination": table["throats"].astype(np.int64),
            "pairs": np.stack([throats["a"], throats["b"]], axis=1).astype(np.int64) if len(throats) else np.zeros((0, 2), np.int64),
            "neck_radius": np.sqrt(throats["neck_sq"].astype(np.float64)), "faces": throats["faces"].astype(np.int64)}


def skeleton_graph(nodes, branches, h=1.0):
    """A skeleton's tables (Voxelizer.Skeleton) as a graph: {"length": float64 [B], steps[0] + sqrt(2) steps[1] + sqrt(3) steps[2] times h, the
    voxel's edge in object units; "len345": int64 [B], the same in SkeletonPrune's integer weights; "pairs": int64 [B, 2], the nodes a <= b of every
    branch (0, 0: a closed cycle); "closed", "spur": bool [B]; "mean_radius", "min_radius": float64 [B], sqrt of w_sum / voxels and of w_min -- for
    weights that are squared radii, a Thickness map's -- times h, NaN where no weights were given (w_max == 0); "degree": int64 [K]; "tip": bool
    [K]}.  Numbers count from 1: node k is row k - 1.  Pure numpy."""
    nodes, branches = np.atleast_1d(np.asarray(nodes, SKELETON_NODE)), np.atleast_1d(np.asarray(branches, SKELETON_BRANCH))
    steps = branches["steps"].astype(np.float64).reshape(-1, 3)
    isteps = branches["steps"].astype(np.int64).reshape(-1, 3)
    voxels = branches["voxels"].astype(np.float64)
    given = branches["w_max"] > 0
    with np.errstate(invalid="ignore", divide="ignore"):
        mean = np.where(given, np.sqrt(branches["w_sum"].astype(np.float64) / voxels), np.nan)
    return {"length": (steps[:, 0] + np.sqrt(2.0) * steps[:, 1] + np.sqrt(3.0) * steps[:, 2]) * float(h),
            "len345": 3 * isteps[:, 0] + 4 * isteps[:, 1] + 5 * isteps[:, 2],
            "pairs": np.stack([branches["a"], branches["b"]], axis=1).astype(np.int64) if len(branches) else np.zeros((0, 2), np.int64),
            "closed": (branches["flags"] & SKELETON_CLOSED) != 0, "spur": (branches["flags"] & SKELETON_SPUR) != 0,
            "mean_radius": mean * float(h), "min_radius": np.where(given, np.sqrt(branches["w_min"].astype(np.float64)), np.nan) * float(h),
            "degree": nodes["degree"].astype(np.int64), "tip": (nodes["voxels"] == 1) & (nodes["degree"] == 1)}


def thickness_voxels(field):
    """A thickness map (ThicknessField: squared radii) in voxels, float32: 2 sqrt(W) - 1 on members, 0 elsewhere -- the diameter of the largest
    voxel-centred ball through the voxel.  A slab k voxels thick reads 2 ceil(k / 2) - 1: balls are centred on voxels, so even thicknesses read
    as the next odd one."""
    W = np.asarray(field)
    return np.where(W > 0, np.float32(2) * np.sqrt(W.astype(np.float32)) - np.float32(1), np.float32(0)).astype(np.float32)


def intrusion_curve(histogram, members=None):
    """The intrusion (drainage) curve of an IntrusionHistogram: (diameter float32 [capSq], share float64 [capSq]) -- for t = 1 .. capSq the
    diameter in voxels of the ball of squared radius t (thickness_voxels) and the share of the members with I >= t: how much of the space a
    ball that large gets into.  members: the members reached or not (AccessInfo: reached + unreached); by default the voxels the histogram
    counts above 0, the members something gets to.  Pure numpy."""
    h = np.asarray(histogram, np.uint64).astype(np.float64)
    t = np.arange(1, len(h), dtype=np.uint32)
    total = float(members) if members is not None else float(h[1:].sum())
    at_least = np.cumsum(h[:0:-1])[::-1]                                # at_least[t - 1] = the voxels with I >= t
    return thickness_voxels(t), (at_least / total if total else np.zeros(len(t)))


def sight_bit(dx, dy, dz):
    """The bit number of direction (dx, dy, dz) in {-1, 0, 1}^3 without 0 in a line-of-sight map's words (include/dxv.h): (dz + 1) * 9 +
    (dy + 1) * 3 + (dx + 1).  The opposite direction has bit 26 - b; Sight(directions=1 << sight_bit(0, 0, 1)) asks for rays travelling up z."""
    if not all(int(d) in (-1, 0, 1) for d in (dx, dy, dz)) or (int(dx), int(dy), int(dz)) == (0, 0, 0):
        raise ValueError(f"sight_bit: ({dx}, {dy}, {dz}) is not one of the 26 lattice directions")
    return (int(dz) + 1) * 9 + (int(dy) + 1) * 3 + int(dx) + 1


def sight_axes(tally):
    """The 13 axes of a SightTally, best pull axis first: a list of {"axis": a, "direction": (dx, dy, dz) of its bit 14 + a, "bits": the
    axis' two bits as a mask, "neither": the members seen along neither of its directions -- the undercut volume of a two-part mould pulled
    along it}, sorted by (neither, axis).  Meaningful for the axes both of whose directions the map was made with (SIGHT_ALL: all).  Pure numpy."""
    neither = np.asarray(tally["neither"], np.uint64)
    rows = []
    for a in range(13):
        b = 14 + a
        rows.append({"axis": a, "direction": (b % 3 - 1, b // 3 % 3 - 1, b // 9 - 1), "bits": (1 << b) | (1 << (26 - b)), "neither": int(neither[a])})
    return sorted(rows, key=lambda r: (r["neither"], r["axis"]))


class Voxelizer:
    """bool-returning calls of the reference become exceptions (DxvError) here."""

    FrameCount = 3  # Content/Voxelizer.h:24

    def __init__(self, device=0):
        self._lib = load_library()
        self._ctx = C.c_void_p()
        if self._lib.dxv_create(C.byref(self._ctx), int(device)):
            raise DxvError(self._lib.dxv_last_error(None).decode())
        self.device = int(device)
        self._frame = 0
        self._lasts = {}
        self._viewports = {}
        self._dist_formats = {}
        # DXV_OPTIONS="key=value,...": options for every context of a process (A/B runs of the tools without touching them)
        import os
        for kv in filter(None, os.environ.get("DXV_OPTIONS", "").split(",")):
            k, val = kv.split("=")
            self.set_option(k.strip(), int(val))

    # ---- lifetime ---------------------------------------------------------------------------
    def close(self):
        if getattr(self, "_ctx", None):
            self._lib.dxv_destroy(self._ctx)
            self._ctx = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc):
        if rc:
            raise DxvError(self._lib.dxv_last_error(self._ctx).decode())

    def _pointer(self, entry):
        """what the entry `entry` hands out for the selected frame (a dxv_*_device_ptr), or the library's refusal as a DxvError"""
        p = getattr(self._lib, entry)(self._ctx)
        if not p:
            raise DxvError(self._lib.dxv_last_error(self._ctx).decode())
        return p

    def _download(self, name, dtype, shape="records", speaks=None, size=None):
        """numpy copy of a product of the selected frame through dxv_<name>_download, sized by dxv_<size or name>_bytes.  shape: "cube", a field
        [n, n, n] of side n = round(cbrt(elements)); "slab", the mesh distance field's [nz, N, N]; "records", a flat array.  A size of 0 does
        not say why: `speaks` is the entry that is called for the message then (a dxv_*_device_ptr, or the one size that speaks), and what it
        refuses is raised; where it refuses nothing the product is an empty table.  Without one the download's own refusal is raised."""
        nbytes = getattr(self._lib, f"dxv_{size or name}_bytes")(self._ctx)
        if not nbytes and speaks:
            self._pointer(speaks)
        count = nbytes // np.dtype(dtype).itemsize
        if shape == "cube":
            n = round(count ** (1.0 / 3.0))
            out = np.empty((n, n, n), dtype)
        elif shape == "slab":
            # the library's own record of the frame's last launch (dxv_get_stats: grid_dim, nz), which is the field's while the field is current
            st = self.stats()
            n, nz = (st["grid_dim"], st["nz"]) if nbytes else (0, 0)
            if n * n * nz != count:
                raise DxvError(f"mesh distance field of {nbytes} bytes does not belong to the frame's last launch ({n}^2 x {nz} voxels)")
            out = np.empty((nz, n, n), dtype)
        else:
            out = np.empty(count, dtype)
        self._check(getattr(self._lib, f"dxv_{name}_download")(self._ctx, out.ctypes.data_as(C.c_void_p), out.nbytes))
        return out

    # ---- reference surface ------------------------------------------------------------------
    def Init(self, fileName, posScale=(0.0, 0.0, 0.0, 1.0), dynamicMesh=False, gridDim=0):
        """Voxelizer::Init (Content/Voxelizer.cpp:30-79) minus the D3D12 arguments."""
        vb, ib, _ = obj_load(fileName)
        return self.InitFromArrays(vb, ib, posScale, dynamicMesh, gridDim)

    def InitFromArrays(self, vb, ib, posScale=(0.0, 0.0, 0.0, 1.0), dynamicMesh=False, gridDim=0):
        """Upload, bound, LBVH -- and, like the reference's Init (Content/Voxelizer.cpp:73), everything else the launches trace
        through: the candidate lists of the reference rule on the map a static scene is launched with, so that the first
        Voxelize costs what every later one costs.  gridDim (the reference's GRID_SIZE, a compile-time constant there,
        Content/Voxelizer.cpp:8): the grid the scene will be voxelized at -- its work queue is then Init-time structure too
        (dxv_prepare_launch) and a Voxelize(gridDim) is one clear + one hardware-dispatched launch; 0: every launch builds its
        queue itself.  dynamicMesh=True (a mesh that is refitted every frame): the LBVH only."""
        self.posScale = tuple(posScale)  # display only in the reference (Voxelizer.cpp:84-87)
        vb = np.ascontiguousarray(vb, np.float32).reshape(-1, 6)
        ib = np.ascontiguousarray(ib, np.uint32).reshape(-1)
        if ib.size % 3:
            raise DxvError("index count is not a multiple of 3")
        self._check(self._lib.dxv_set_mesh(self._ctx, vb, len(vb), ib, ib.size // 3))
        self._check(self._lib.dxv_build(self._ctx))
        if not dynamicMesh:
            self._check(self._lib.dxv_build_lists_for_grid(self._ctx, int(gridDim)))
        return True

    def PrepareLaunch(self, gridDim, z0=0, nz=None):
        """dxv_prepare_launch: the work queue of slices [z0, z0 + nz) of a gridDim^3 grid, built now and kept with the scene."""
        nz = gridDim - z0 if nz is None else nz
        self._check(self._lib.dxv_prepare_launch(self._ctx, int(gridDim), int(z0), int(nz)))
        return True

    def PrepareLaunchInterleaved(self, gridDim, rank, world, zblock=8):
        """dxv_prepare_launch_interleaved: the same for this rank's share of the block-cyclic partition."""
        self._check(self._lib.dxv_prepare_launch_interleaved(self._ctx, int(gridDim), int(rank), int(world), int(zblock)))
        return True

    def InitDynamic(self, vb, ib, posScale=(0.0, 0.0, 0.0, 1.0)):
        return self.InitFromArrays(vb, ib, posScale, dynamicMesh=True)

    def UpdateVertices(self, vb, refit=True):
        """Animated vertices on fixed topology: upload + refit of the existing hierarchy (N4)."""
        vb = np.ascontiguousarray(vb, np.float32).reshape(-1, 6)
        self._check(self._lib.dxv_update_vertices(self._ctx, vb, len(vb)))
        if refit:
            self._check(self._lib.dxv_refit(self._ctx))
        return True

    def Refit(self):
        """dxv_refit on its own: after UpdateVertices(vb, refit=False), whose upload overlapped a launch still in flight."""
        self._check(self._lib.dxv_refit(self._ctx))
        return True

    def UpdateVerticesDevice(self, device_ptr, num_verts, refit=True):
        """The same from a device buffer (6 floats per vertex on this GPU, e.g. a torch tensor's data_ptr()): a mesh animated
        on the GPU never passes through the host."""
        self._check(self._lib.dxv_update_vertices_device(self._ctx, C.c_void_p(int(device_ptr)), int(num_verts)))
        if refit:
            self._check(self._lib.dxv_refit(self._ctx))
        return True

    def SetFrame(self, frameIndex):
        """The frame (0 .. FrameCount-1) the following Voxelize / Sync / Grid / Texels / Render / stats calls refer
        to: the reference's frameIndex argument (Content/Voxelizer.h:20-22) and its m_grids[FrameCount] (:110)."""
        self._check(self._lib.dxv_set_frame(self._ctx, int(frameIndex)))
        self._frame = int(frameIndex)

    def Voxelize(self, gridDim, mode=MODE_REFERENCE, z0=0, nz=None, sync=True, frameIndex=None):
        """Voxelizer::voxelize(pCommandList, frameIndex) (Content/Voxelizer.cpp:351-369) with gridDim as a parameter."""
        if frameIndex is not None:
            self.SetFrame(frameIndex)
        nz = gridDim - z0 if nz is None else nz
        fn = self._lib.dxv_voxelize if sync else self._lib.dxv_voxelize_async
        self._check(fn(self._ctx, int(gridDim), int(mode), int(z0), int(nz)))
        self._lasts[self._frame] = (int(gridDim), int(nz))
        return True

    def VoxelizeInterleaved(self, gridDim, rank, world, zblock=8, mode=MODE_REFERENCE, sync=True, frameIndex=None):
        """This rank's share of a block-cyclic Z partition (dxv_voxelize_interleaved)."""
        if frameIndex is not None:
            self.SetFrame(frameIndex)
        fn = self._lib.dxv_voxelize_interleaved if sync else self._lib.dxv_voxelize_interleaved_async
        self._check(fn(self._ctx, int(gridDim), int(mode), int(rank), int(world), int(zblock)))
        self._lasts[self._frame] = (int(gridDim), int(gridDim) // int(world))
        return True

    def Sync(self):
        self._check(self._lib.dxv_sync(self._ctx))

    def SyncAll(self):
        """Wait for the launches of every frame (dxv_sync_all)."""
        self._check(self._lib.dxv_sync_all(self._ctx))

    @property
    def _last(self):
        return self._lasts.get(self._frame)

    # ---- the grid's consumer (Voxelizer::UpdateFrame + Render's ray-cast pass) -----------------
    def Render(self, eyePt, viewProj, width=1280, height=720, posScale=None):
        """uint8 [height, width, 4] R8G8B8A8 image of the last full grid (dxv_render)."""
        eye = np.ascontiguousarray(eyePt, np.float32).reshape(3)
        vp = np.ascontiguousarray(viewProj, np.float32).reshape(16)
        ps = None if posScale is None else np.ascontiguousarray(posScale, np.float32).ctypes.data_as(C.c_void_p)
        out = np.empty((int(height), int(width), 4), np.uint8)
        self._check(self._lib.dxv_render(self._ctx, eye, vp, ps, int(width), int(height), out.ctypes.data_as(C.c_void_p)))
        return out

    # ---- the reference's frame loop: per-frame constants, ray-cast into a device render target ----
    def UpdateFrame(self, frameIndex, eyePt, viewProj, width, height, posScale=None):
        """Voxelizer::UpdateFrame(frameIndex, eyePt, viewProj) (Content/Voxelizer.cpp:81-106): frame frameIndex's ray-cast
        constants for a width x height viewport (dxv_update_frame), kept by the frame until its next UpdateFrame."""
        self.SetFrame(frameIndex)
        eye = np.ascontiguousarray(eyePt, np.float32).reshape(3)
        vp = np.ascontiguousarray(viewProj, np.float32).reshape(16)
        ps = None if posScale is None else np.ascontiguousarray(posScale, np.float32).reshape(4)
        self._check(self._lib.dxv_update_frame(self._ctx, eye, vp, None if ps is None else ps.ctypes.data_as(C.c_void_p),
                                               int(width), int(height)))
        self._viewports[self._frame] = (int(height), int(width))
        return True

    def RenderAsync(self, target, frameIndex=None):
        """renderRayCast(frameIndex) (Content/Voxelizer.cpp:371-399) into `target` on the GPU, enqueued behind the frame's launch
        (dxv_render_async).  target: anything with data_ptr(), shape (H, W, 4) of the frame's viewport, dtype uint8, and rows
        at least W * 4 bytes apart -- a torch tensor on this device, or a row slice big[:, :W] of a wider one.  Ordering the target
        against other streams is the caller's (WaitFrameOn, Sync)."""
        if frameIndex is not None:
            self.SetFrame(frameIndex)
        shape = tuple(int(n) for n in target.shape)
        if len(shape) != 3 or shape[2] != 4 or not str(target.dtype).endswith("uint8"):
            raise DxvError(f"RenderAsync: target must be uint8 of shape (H, W, 4), got {target.dtype} {shape}")
        want = self._viewports.get(self._frame)
        if want is not None and shape[:2] != want:
            raise DxvError(f"RenderAsync: target is {shape[0]} x {shape[1]}, frame {self._frame}'s viewport {want[0]} x {want[1]}")
        stride = tuple(int(n) for n in target.stride()) if callable(getattr(target, "stride", None)) else (shape[1] * 4, 4, 1)
        if stride[1:] != (4, 1):
            raise DxvError(f"RenderAsync: the texels of a row must be contiguous (strides {stride})")
        pitch = stride[0] * (int(target.element_size()) if hasattr(target, "element_size") else 1)
        self._check(self._lib.dxv_render_async(self._ctx, C.c_void_p(int(target.data_ptr())), pitch))
        return True

    def WaitFrameOn(self, stream_handle):
        """Make a consumer's stream (a hipStream_t handle, e.g. torch's stream.cuda_stream, or an object with that attribute) wait
        on the device for everything enqueued on the selected frame so far (dxv_stream_wait_frame)."""
        handle = getattr(stream_handle, "cuda_stream", stream_handle)
        self._check(self._lib.dxv_stream_wait_frame(self._ctx, C.c_void_p(int(handle)) if handle else None))
        return True

    # ---- results ----------------------------------------------------------------------------
    def Grid(self):
        """uint8 [nz, N, N] (z, y top->bottom, x) copy of the device grid."""
        n, nz = self._last
        out = np.empty((nz, n, n), np.uint8)
        self._check(self._lib.dxv_grid_download(self._ctx, out.ctypes.data_as(C.c_void_p), out.nbytes))
        return out

    def GridBits(self, out=None):
        """The grid as one bit per voxel, packed on the device (dxv_grid_download_packed): uint8
        [ceil(nz*N*N/8)], voxel 8j+i in bit i of byte j, set iff the voxel's byte is non-zero
        == np.packbits(Grid().ravel(), bitorder="little") (numpy, too, takes every non-zero byte
        for 1).  `out` may be any writable uint8 buffer of that size, e.g. pinned."""
        nbytes = self._lib.dxv_grid_packed_bytes(self._ctx)
        if out is None:
            out = np.empty(nbytes, np.uint8)
        ptr = out.ctypes.data_as(C.c_void_p) if isinstance(out, np.ndarray) else C.c_void_p(out.data_ptr())
        size = out.nbytes if isinstance(out, np.ndarray) else out.numel() * out.element_size()
        self._check(self._lib.dxv_grid_download_packed(self._ctx, ptr, size))
        return out

    def Texels(self):
        n, nz = self._last
        out = np.empty((nz, n, n), np.uint32)
        self._check(self._lib.dxv_texels_download(self._ctx, out.ctypes.data_as(C.c_void_p), out.nbytes))
        return out

    def EnableTexels(self, on=True):
        self._check(self._lib.dxv_enable_texels(self._ctx, int(bool(on))))

    def CountSolid(self):
        """Solid voxels of the selected frame's grid, counted on the device (dxv_grid_count); a voxel is solid iff its byte is
        non-zero == np.count_nonzero(Grid())."""
        v = C.c_uint64()
        self._check(self._lib.dxv_grid_count(self._ctx, C.byref(v)))
        return v.value

    def grid_device_ptr(self, writable=True):
        """Device pointer of the selected frame's grid.  writable=True (dxv_grid_device_ptr) tells the library that the caller
        may write through it at any later time: the frame's launches then clear the grid every time.  writable=False
        (dxv_grid_device_ptr_ro) is for consumers that only read."""
        if writable:
            return self._lib.dxv_grid_device_ptr(self._ctx)
        return self._lib.dxv_grid_device_ptr_ro(self._ctx)

    # ---- the distance field of the frame's grid ---------------------------------------------------
    def DistanceField(self, format=DIST_F32, sync=True, frameIndex=None):
        """The exact signed distance field of the selected frame's whole grid (dxv_distance / dxv_distance_async): negative inside,
        voxel units, centre to centre.  format DIST_SQ_I32: int32 s * d2; DIST_F32: float32 s * sqrt(d2).  sync=True returns it as a
        numpy array [N, N, N] (z, y, x); sync=False only enqueues it behind the frame's launch and returns True (distance_device_ptr,
        Distance after a Sync)."""
        if frameIndex is not None:
            self.SetFrame(frameIndex)
        if format not in (DIST_SQ_I32, DIST_F32):
            raise DxvError(f"DistanceField: unknown format {format!r} (DIST_SQ_I32 = 0, DIST_F32 = 1)")
        fn = self._lib.dxv_distance if sync else self._lib.dxv_distance_async
        self._check(fn(self._ctx, int(format)))
        self._dist_formats[self._frame] = int(format)
        return self.Distance() if sync else True

    def Distance(self):
        """numpy copy of the selected frame's field (dxv_distance_download; synchronises the frame)."""
        return self._download("distance", np.float32 if self._dist_formats.get(self._frame) == DIST_F32 else np.int32, "cube")

    def distance_device_ptr(self):
        """Device pointer of the selected frame's field (dxv_distance_device_ptr), for consumers on the GPU; raises where the
        library refuses (no field yet, or the frame was launched again since)."""
        return self._pointer("dxv_distance_device_ptr")

    def distance_ms(self):
        """Device time of the selected frame's last field, read at the frame's Sync (dxv_distance_ms)."""
        ms = C.c_float()
        self._check(self._lib.dxv_distance_ms(self._ctx, C.byref(ms)))
        return ms.value

    # ---- the distance from the voxel centres to the mesh -------------------------------------------
    def MeshDistanceField(self, format=MDIST_VOXELS_F32, band=0, triangles=False, sync=True, frameIndex=None):
        """The exact Euclidean distance from every voxel centre of the selected frame's last launch (the whole grid or a contiguous slab)
        to the nearest triangle, negative where the frame's grid byte is non-zero (dxv_mesh_distance / dxv_mesh_distance_async).
        format MDIST_VOXELS_F32: voxel units like DistanceField; MDIST_UNITS_F32: normalised units.  band > 0 caps the distance at that
        many voxels; triangles=True keeps the nearest triangle's index per voxel (MeshDistanceTriangles).  sync=True returns the field as
        a float32 numpy array [nz, N, N] (z, y, x); sync=False only enqueues it behind the frame's launch and returns True."""
        if frameIndex is not None:
            self.SetFrame(frameIndex)
        if format not in (MDIST_VOXELS_F32, MDIST_UNITS_F32):
            raise DxvError(f"MeshDistanceField: unknown format {format!r} (MDIST_VOXELS_F32 = 0, MDIST_UNITS_F32 = 1)")
        fn = self._lib.dxv_mesh_distance if sync else self._lib.dxv_mesh_distance_async
        self._check(fn(self._ctx, int(format), int(band), 1 if triangles else 0))
        return self.MeshDistance() if sync else True

    def MeshDistance(self):
        """numpy copy of the selected frame's mesh distance field (dxv_mesh_distance_download; synchronises the frame)."""
        return self._download("mesh_distance", np.float32, "slab")

    def MeshDistanceTriangles(self):
        """numpy copy (uint32) of the nearest triangle per voxel, 0xffffffff beyond the band (dxv_mesh_distance_triangles_download); raises
        when the field was made without them."""
        return self._download("mesh_distance_triangles", np.uint32, "slab", size="mesh_distance")

    def mesh_distance_device_ptr(self):
        """Device pointer of the selected frame's mesh distance field (dxv_mesh_distance_device_ptr); raises where the library refuses
        (no field yet, or the frame was launched or filled again since)."""
        return self._pointer("dxv_mesh_distance_device_ptr")

    def mesh_distance_ms(self):
        """Device time of the selected frame's last mesh distance field, read at the frame's Sync (dxv_mesh_distance_ms)."""
        ms = C.c_float()
        self._check(self._lib.dxv_mesh_distance_ms(self._ctx, C.byref(ms)))
        return ms.value

    # ---- the isosurface of one of the frame's fields ------------------------------------------------
    def Isosurface(self, source=ISO_MESH_DISTANCE, iso=0.0, space=ISO_SPACE_OBJECT, sync=True, frameIndex=None):
        """A closed triangle mesh of the level `iso` of the selected frame's mesh distance field (ISO_MESH_DISTANCE) or of its grid distance
        field in DIST_F32 (ISO_GRID_DISTANCE), by naive Surface Nets on the device (dxv_isosurface / dxv_isosurface_async); iso in the
        field's unit.  space ISO_SPACE_OBJECT: the space of the mesh Init was given, so (vb, ib) go back into InitFromArrays as they are;
        ISO_SPACE_VOXELS: voxel index space.  sync=True returns (vb [V, 6] float32 {pos, nrm}, ib [3T] uint32); sync=False only enqueues
        the emit pass (the call still reads the mesh's two sizes once) and returns True (IsosurfaceMesh after a Sync)."""
        if frameIndex is not None:
            self.SetFrame(frameIndex)
        if source not in (ISO_MESH_DISTANCE, ISO_GRID_DISTANCE):
            raise DxvError(f"Isosurface: unknown source {source!r} (ISO_MESH_DISTANCE = 0, ISO_GRID_DISTANCE = 1)")
        if space not in (ISO_SPACE_VOXELS, ISO_SPACE_OBJECT):
            raise DxvError(f"Isosurface: unknown space {space!r} (ISO_SPACE_VOXELS = 0, ISO_SPACE_OBJECT = 1)")
        fn = self._lib.dxv_isosurface if sync else self._lib.dxv_isosurface_async
        self._check(fn(self._ctx, int(source), float(iso), int(space)))
        return self.IsosurfaceMesh() if sync else True

    def IsosurfaceCounts(self):
        """(vertices, triangles) of the selected frame's mesh (dxv_isosurface_counts); raises where the library refuses (no mesh yet, or
        the frame was launched or filled again since)."""
        nv, nt = C.c_uint32(), C.c_uint32()
        self._check(self._lib.dxv_isosurface_counts(self._ctx, C.byref(nv), C.byref(nt)))
        return nv.value, nt.value

    def IsosurfaceMesh(self):
        """numpy copies (vb [V, 6] float32, ib [3T] uint32) of the selected frame's mesh (dxv_isosurface_*_download; synchronises the frame)."""
        nv, nt = self.IsosurfaceCounts()
        vb, ib = np.empty((nv, 6), np.float32), np.empty(3 * nt, np.uint32)
        self._check(self._lib.dxv_isosurface_vertices_download(self._ctx, vb.ctypes.data_as(C.c_void_p), vb.nbytes))
        self._check(self._lib.dxv_isosurface_indices_download(self._ctx, ib.ctypes.data_as(C.c_void_p), ib.nbytes))
        return vb, ib

    def isosurface_device_ptrs(self):
        """Device pointers (vertices, indices) of the selected frame's mesh, for consumers on the GPU; (None, None) for the empty mesh;
        raises where the library refuses."""
        self.IsosurfaceCounts()
        return self._lib.dxv_isosurface_vertices_device_ptr(self._ctx), self._lib.dxv_isosurface_indices_device_ptr(self._ctx)

    def isosurface_ms(self):
        """Device time of the selected frame's last extraction, read at the frame's Sync (dxv_isosurface_ms)."""
        ms = C.c_float()
        self._check(self._lib.dxv_isosurface_ms(self._ctx, C.byref(ms)))
        return ms.value

    # ---- the sparse voxel octree of the frame's grid ------------------------------------------------
    def Octree(self, sync=True, frameIndex=None):
        """The sparse voxel octree of the selected frame's whole grid, built on the device (dxv_octree / dxv_octree_async; include/dxv.h has
        the rule): one 8-byte node for the root and for every mixed cell, full and empty cells have none.  sync=True returns (nodes [n, 2]
        uint32 {word0, word1}, level_first [L + 1]); sync=False only enqueues the emit pass (the call still reads the level totals once)
        and returns True (OctreeNodes after a Sync)."""
        if frameIndex is not None:
            self.SetFrame(frameIndex)
        fn = self._lib.dxv_octree if sync else self._lib.dxv_octree_async
        self._check(fn(self._ctx))
        return self.OctreeNodes() if sync else True

    def OctreeInfo(self):
        """(levels L, nodes, level_first [L + 1]) of the selected frame's tree (dxv_octree_info); raises where the library refuses (no tree
        yet, or the frame was launched, filled or expanded again since)."""
        levels, nodes, first = C.c_uint32(), C.c_uint32(), (C.c_uint32 * 12)()
        self._check(self._lib.dxv_octree_info(self._ctx, C.byref(levels), C.byref(nodes), first))
        return levels.value, nodes.value, [int(v) for v in first[:levels.value + 1]]

    def OctreeNodes(self):
        """numpy copy (nodes [n, 2] uint32, level_first) of the selected frame's tree (dxv_octree_download; synchronises the frame)."""
        _, _, first = self.OctreeInfo()
        return self._download("octree", np.uint32).reshape(-1, 2), first

    def octree_device_ptr(self):
        """Device pointer of the selected frame's nodes (dxv_octree_device_ptr), for consumers on the GPU; raises where the library refuses."""
        return self._pointer("dxv_octree_device_ptr")

    def octree_bytes(self):
        return self._lib.dxv_octree_bytes(self._ctx)

    def octree_ms(self):
        """Device time of the selected frame's last octree build, read at the frame's Sync (dxv_octree_ms)."""
        ms = C.c_float()
        self._check(self._lib.dxv_octree_ms(self._ctx, C.byref(ms)))
        return ms.value

    def OctreeExpand(self, nodes=None, levels=None, count=None, sync=True, frameIndex=None):
        """Write the selected frame's whole grid from an octree, every voxel 0 or 1 (dxv_octree_expand / dxv_octree_expand_async).
        nodes=None: the frame's own current tree.  Otherwise a tree on this device: a torch tensor of uint32 / int32 words, two per node
        (anything with data_ptr() and numel()), or a device pointer with count = its nodes; levels = the tree's L, which must be the L of
        the frame's grid.  The tree is not trusted: an index it holds that cannot be followed fails the frame's next Sync."""
        if frameIndex is not None:
            self.SetFrame(frameIndex)
        fn = self._lib.dxv_octree_expand if sync else self._lib.dxv_octree_expand_async
        if nodes is None:
            self._check(fn(self._ctx, None, 0, 0))
            return True
        if hasattr(nodes, "data_ptr"):
            if int(nodes.element_size()) != 4 or int(nodes.numel()) % 2 or not nodes.is_contiguous():
                raise DxvError(f"OctreeExpand: nodes must be contiguous 32-bit words, two per node, got {nodes.dtype} {tuple(nodes.shape)}")
            ptr, count = int(nodes.data_ptr()), int(nodes.numel()) // 2 if count is None else int(count)
        else:
            if count is None:
                raise DxvError("OctreeExpand: a device pointer needs count = the number of its nodes")
            ptr = int(nodes)
        if levels is None:
            raise DxvError("OctreeExpand: a caller's tree needs levels = its L")
        self._check(fn(self._ctx, C.c_void_p(ptr), int(count), int(levels)))
        return True

    # ---- the connected components of the frame's grid ----------------------------------------------
    def Components(self, of=COMP_SOLID, connectivity=6, sync=True, frameIndex=None):
        """Label the connected components of the selected frame's whole grid on the device (dxv_components / dxv_components_async; include/dxv.h
        has the rule): of = COMP_SOLID the non-zero voxels, COMP_EMPTY the zero ones; connectivity 6 or 26; components numbered 1 .. K by their
        smallest linear index.  sync=True returns (labels [N, N, N] uint32, table), the table a structured array with fields first, voxels,
        lo, hi, flags; sync=False only enqueues the stats pass (the call still reads K once) and returns True."""
        if frameIndex is not None:
            self.SetFrame(frameIndex)
        fn = self._lib.dxv_components if sync else self._lib.dxv_components_async
        self._check(fn(self._ctx, int(of), int(connectivity)))
        return (self.ComponentLabels(), self.ComponentTable()) if sync else True

    def components_info(self):
        """(K, of, connectivity) of the selected frame's labelling (dxv_components_info); raises where the library refuses (none yet, or stale)."""
        count, of, conn = C.c_uint32(), C.c_int(), C.c_int()
        self._check(self._lib.dxv_components_info(self._ctx, C.byref(count), C.byref(of), C.byref(conn)))
        return count.value, of.value, conn.value

    def ComponentLabels(self):
        """numpy copy [N, N, N] uint32 of the selected frame's labels (dxv_components_labels_download; synchronises the frame)."""
        self.components_info()                                          # (raises where there are none, or stale ones)
        return self._download("components_labels", np.uint32, "cube")

    def ComponentTable(self):
        """numpy copy [K] of the selected frame's table, dtype COMP_RECORD (dxv_components_table_download; synchronises the frame)."""
        self.components_info()
        return self._download("components_table", COMP_RECORD)

    def component_device_ptrs(self):
        """(labels, table) device pointers of the selected frame's labelling, for consumers on the GPU; the table's is None when K = 0."""
        return self._pointer("dxv_components_labels_device_ptr"), self._lib.dxv_components_table_device_ptr(self._ctx)

    def components_ms(self):
        """Device time of the selected frame's last labelling, read at the frame's Sync (dxv_components_ms)."""
        ms = C.c_float()
        self._check(self._lib.dxv_components_ms(self._ctx, C.byref(ms)))
        return ms.value

    # ---- the integral measures of the frame's labelling -----------------------------------------------
    def Measure(self, sync=True, frameIndex=None):
        """Measure every component of the selected frame's current labelling on the device (dxv_measure / dxv_measure_async; include/dxv.h has
        the rule): voxels, first and second moments of the voxel indices, exposed faces and the Euler characteristic by the labelling's
        connectivity, K + 1 records with record 0 the sum of the others.  sync=True returns MeasureTable(); sync=False only enqueues it."""
        if frameIndex is not None:
            self.SetFrame(frameIndex)
        fn = self._lib.dxv_measure if sync else self._lib.dxv_measure_async
        self._check(fn(self._ctx))
        return self.MeasureTable() if sync else True

    def MeasureTable(self):
        """numpy copy [K + 1] of the selected frame's measures, dtype MEASURE_RECORD (dxv_measure_table_download; synchronises the frame)."""
        return self._download("measure_table", MEASURE_RECORD, speaks="dxv_measure_table_bytes")

    def measure_device_ptr(self):
        """Device pointer of the selected frame's measures, (K + 1) * 96 bytes, for consumers on the GPU."""
        return self._pointer("dxv_measure_table_device_ptr")

    def measure_ms(self):
        """Device time of the selected frame's last measure, read at the frame's Sync (dxv_measure_ms)."""
        ms = C.c_float()
        self._check(self._lib.dxv_measure_ms(self._ctx, C.byref(ms)))
        return ms.value

    def Betti(self, frameIndex=None):
        """(b0, b1, b2) of the selected frame's solid as a complex of closed unit cubes: pieces, handles, cavities.  Components(COMP_EMPTY, 6)
        gives b2, the empty components that do not reach the grid's border; Components(COMP_SOLID, 26) and Measure give b0 = K and the
        Euler number, and b1 = b0 + b2 - euler.  The solid labelling and its measure stay current."""
        if frameIndex is not None:
            self.SetFrame(frameIndex)
        _, empty = self.Components(COMP_EMPTY, 6)
        b2 = int(np.count_nonzero((empty["flags"] & 1) == 0))
        self._check(self._lib.dxv_components(self._ctx, COMP_SOLID, 26))
        b0 = self.components_info()[0]
        return betti_numbers(b0, b2, int(self.Measure()[0]["euler"]))

    # ---- the local thickness of the frame's grid ------------------------------------------------------
    def Thickness(self, of=COMP_SOLID, capSq=4096, sync=True, frameIndex=None):
        """The exact local thickness of the selected frame's whole grid on the device (dxv_thickness / dxv_thickness_async; include/dxv.h has the
        rule): per member voxel -- of = COMP_SOLID the non-zero voxels, COMP_EMPTY the zero ones -- the largest R(c) = min(D2(c), capSq) of a
        member c whose open ball { |p - c|^2 < R(c) } holds the voxel, 0 for the others; 2 <= capSq <= 4096.  The minimum wall of a part, and
        with COMP_EMPTY channel widths and pore sizes.  The grid and the frame's other products stay as they are.  sync=True returns
        ThicknessField(); sync=False only enqueues it."""
        if frameIndex is not None:
            self.SetFrame(frameIndex)
        fn = self._lib.dxv_thickness if sync else self._lib.dxv_thickness_async
        self._check(fn(self._ctx, int(of), int(capSq)))
        return self.ThicknessField() if sync else True

    def ThicknessField(self):
        """numpy copy uint32 [N, N, N] (z, y, x) of the selected frame's thickness map, squared radii (dxv_thickness_download; synchronises
        the frame); thickness_voxels turns it into voxels."""
        return self._download("thickness", np.uint32, "cube", speaks="dxv_thickness_device_ptr")

    def ThicknessHistogram(self):
        """numpy copy uint64 [capSq + 1] of the selected frame's thickness histogram: bin v the voxels with W == v, bin 0 those that are no
        members (dxv_thickness_histogram_download; synchronises the frame).  Its first non-zero bin above 0 is the minimum wall."""
        return self._download("thickness_histogram", np.uint64, speaks="dxv_thickness_device_ptr")

    def thickness_device_ptr(self):
        """Device pointer of the selected frame's thickness map, 4 * N^3 bytes, for consumers on the GPU."""
        return self._pointer("dxv_thickness_device_ptr")

    def ThicknessInfo(self):
        """(ms, centres_painted, work_items) of the selected frame's last thickness as of its last Sync (dxv_thickness_info)."""
        ms, centres, items = C.c_float(), C.c_uint64(), C.c_uint64()
        self._check(self._lib.dxv_thickness_info(self._ctx, C.byref(ms), C.byref(centres), C.byref(items)))
        return ms.value, centres.value, items.value

    def thickness_stage_info(self):
        """({stage: ms}, voxels_tested, atomics_sent) of the selected frame's last thickness as of its last Sync (dxv_thickness_stage_info): the
        six stages' device times, the voxels the paint loaded and compared, the atomic maxima it sent (which vary from run to run)."""
        ms, tested, sent = (C.c_float * 6)(), C.c_uint64(), C.c_uint64()
        self._check(self._lib.dxv_thickness_stage_info(self._ctx, ms, C.byref(tested), C.byref(sent)))
        return dict(zip(("field", "top", "cull", "select", "paint", "histogram"), (float(m) for m in ms))), tested.value, sent.value

    # ---- the maximal-ball partition of the frame's grid --------------------------------------------------
    def Partition(self, of=COMP_SOLID, capSq=4096, throats=True, sync=True, frameIndex=None):
        """The maximal-ball partition of the selected frame's whole grid on the device (dxv_partition / dxv_partition_async; include/dxv.h has
        the rule): every member voxel -- of = COMP_SOLID the non-zero voxels, COMP_EMPTY the zero ones -- points to the highest voxel of its own
        closed ball of radius^2 R = min(D2, capSq), by R and then by the smaller index; the roots of that forest are the bodies, a region is the
        family of one root, a throat is where two families share faces; 1 <= capSq <= 4096.  With COMP_EMPTY pores and throats, with
        COMP_SOLID lobes and necks.  The grid and the frame's other products stay as they are.  sync=True returns (PartitionLabels(),
        PartitionTable(), PartitionThroats() or None without throats); sync=False only enqueues it -- the call still waits for its own counts."""
        if frameIndex is not None:
            self.SetFrame(frameIndex)
        fn = self._lib.dxv_partition if sync else self._lib.dxv_partition_async
        self._check(fn(self._ctx, int(of), int(capSq), 1 if throats else 0))
        return (self.PartitionLabels(), self.PartitionTable(), self.PartitionThroats() if throats else None) if sync else True

    def PartitionLabels(self):
        """numpy copy uint32 [N, N, N] (z, y, x) of the selected frame's region labels, 0 off the members (dxv_partition_labels_download;
        synchronises the frame)."""
        return self._download("partition_labels", np.uint32, "cube", speaks="dxv_partition_labels_device_ptr")

    def PartitionTable(self):
        """numpy copy [K] of the selected frame's regions, dtype PART_REGION (dxv_partition_table_download; synchronises the frame)."""
        return self._download("partition_table", PART_REGION, speaks="dxv_partition_labels_device_ptr")

    def PartitionThroats(self):
        """numpy copy [T] of the selected frame's throats, dtype PART_THROAT (dxv_partition_throats_download; synchronises the frame); an
        error for a partition made without them."""
        return self._download("partition_throats", PART_THROAT)

    def partition_device_ptrs(self):
        """(labels, table, throats) device pointers of the selected frame's partition, for consumers on the GPU; the table's is None when K = 0,
        the throats' when T = 0 or when it was made without them."""
        return (self._pointer("dxv_partition_labels_device_ptr"), self._lib.dxv_partition_table_device_ptr(self._ctx),
                self._lib.dxv_partition_throats_device_ptr(self._ctx))

    def PartitionInfo(self):
        """(ms, regions, throats, interface_faces) of the selected frame's last partition as of its last Sync (dxv_partition_info)."""
        ms, regions, throats, faces = C.c_float(), C.c_uint32(), C.c_uint32(), C.c_uint64()
        self._check(self._lib.dxv_partition_info(self._ctx, C.byref(ms), C.byref(regions), C.byref(throats), C.byref(faces)))
        return ms.value, regions.value, throats.value, faces.value

    def partition_stage_info(self):
        """({stage: ms}, cells_tested, voxels_tested) of the selected frame's last partition as of its last Sync (dxv_partition_stage_info): the
        six stages' device times and the mip cells and voxels the parent search tested, under option partstages = 1 (else all 0)."""
        ms, cells, voxels = (C.c_float * 6)(), C.c_uint64(), C.c_uint64()
        self._check(self._lib.dxv_partition_stage_info(self._ctx, ms, C.byref(cells), C.byref(voxels)))
        return dict(zip(("field", "keys", "search", "roots", "regions", "throats"), (float(m) for m in ms))), cells.value, voxels.value

    # ---- the skeleton graph of the frame's grid ------------------------------------------------------------
    def Skeleton(self, weights=None, sync=True, frameIndex=None):
        """The skeleton graph of the selected frame's whole grid on the device (dxv_skeleton / dxv_skeleton_async; include/dxv.h has the rule):
        the members with two members among their 26 neighbours are curve voxels, the others node voxels; a node is a 26-connected cluster of node
        voxels, a branch one of curve voxels -- a path between two attachments to nodes, or a closed cycle.  weights: None, or N^3 uint32 on the
        device laid out like the grid -- a torch tensor of a 4-byte integer dtype or a pointer, for example another frame's
        thickness_device_ptr() -- whose minimum, maximum and sum along every branch go into its record.  A graph of the shape for a grid Thin has
        left.  The grid and the frame's other products stay as they are.  sync=True returns (SkeletonLabels(), SkeletonNodes(),
        SkeletonBranches()); sync=False only enqueues it -- the call still waits for its own counts, and the caller keeps the weights alive and
        unchanged until the frame has been synchronised."""
        if frameIndex is not None:
            self.SetFrame(frameIndex)
        ptr, keep = None, None
        if weights is not None:
            if hasattr(weights, "data_ptr"):
                import torch
                if not weights.is_cuda or weights.element_size() != 4 or weights.is_floating_point() or not weights.is_contiguous():
                    raise DxvError("Skeleton: a weight tensor must be a contiguous 4-byte integer tensor on the device")
                n = self.stats()["grid_dim"]
                if weights.numel() != n ** 3:
                    raise DxvError(f"Skeleton: the weight tensor has {weights.numel()} elements, the grid has {n ** 3} voxels")
                torch.cuda.current_stream(weights.device).synchronize()   # (its writer is ordered before the frame's stream reads it)
                ptr, keep = C.c_void_p(weights.data_ptr()), weights
            else:
                ptr = C.c_void_p(int(weights))
        fn = self._lib.dxv_skeleton if sync else self._lib.dxv_skeleton_async
        self._check(fn(self._ctx, ptr))
        del keep
        return (self.SkeletonLabels(), self.SkeletonNodes(), self.SkeletonBranches()) if sync else True

    def SkeletonLabels(self):
        """numpy copy uint32 [N, N, N] (z, y, x) of the selected frame's skeleton labels: 0 off the members, k on node k, SKELETON_BRANCH_BIT | b on
        branch b (dxv_skeleton_labels_download; synchronises the frame)."""
        return self._download("skeleton_labels", np.uint32, "cube", speaks="dxv_skeleton_labels_device_ptr")

    def SkeletonNodes(self):
        """numpy copy [K] of the selected frame's nodes, dtype SKELETON_NODE (dxv_skeleton_nodes_download; synchronises the frame)."""
        return self._download("skeleton_nodes", SKELETON_NODE, speaks="dxv_skeleton_labels_device_ptr")

    def SkeletonBranches(self):
        """numpy copy [B] of the selected frame's branches, dtype SKELETON_BRANCH (dxv_skeleton_branches_download; synchronises the frame)."""
        return self._download("skeleton_branches", SKELETON_BRANCH, speaks="dxv_skeleton_labels_device_ptr")

    def skeleton_device_ptrs(self):
        """(labels, nodes, branches) device pointers of the selected frame's skeleton, for consumers on the GPU; the nodes' is None when K = 0, the
        branches' when B = 0."""
        return (self._pointer("dxv_skeleton_labels_device_ptr"), self._lib.dxv_skeleton_nodes_device_ptr(self._ctx),
                self._lib.dxv_skeleton_branches_device_ptr(self._ctx))

    def SkeletonInfo(self):
        """{ms, nodes, branches, end_voxels, curve_voxels, junction_voxels} of the selected frame's last skeleton as of its last Sync
        (dxv_skeleton_info): the members with at most one, with two and with three or more members among their 26 neighbours."""
        ms, nodes, branches = C.c_float(), C.c_uint32(), C.c_uint32()
        ends, curve, junctions = C.c_uint64(), C.c_uint64(), C.c_uint64()
        self._check(self._lib.dxv_skeleton_info(self._ctx, C.byref(ms), C.byref(nodes), C.byref(branches), C.byref(ends), C.byref(curve), C.byref(junctions)))
        return {"ms": ms.value, "nodes": nodes.value, "branches": branches.value, "end_voxels": ends.value, "curve_voxels": curve.value, "junction_voxels": junctions.value}

    def SkeletonPrune(self, max_len345, sync=True):
        """Remove short spurs from the selected frame's grid in place, from its current skeleton (dxv_skeleton_prune / _async): every branch with
        exactly one tip -- a node of one voxel and degree 1 -- at an end and 3 steps[0] + 4 steps[1] + 5 steps[2] <= max_len345 goes, with that
        tip.  The skeleton is stale afterwards; the recipe is Thin; Skeleton; SkeletonPrune(L); Thin; Skeleton."""
        fn = self._lib.dxv_skeleton_prune if sync else self._lib.dxv_skeleton_prune_async
        self._check(fn(self._ctx, int(max_len345)))
        return True

    def SkeletonPruneInfo(self):
        """(branches_removed, voxels_removed) of the selected frame's last SkeletonPrune as of its last Sync (dxv_skeleton_prune_info)."""
        branches, voxels = C.c_uint32(), C.c_uint64()
        self._check(self._lib.dxv_skeleton_prune_info(self._ctx, C.byref(branches), C.byref(voxels)))
        return branches.value, voxels.value

    # ---- the geodesic distance inside the frame's grid ---------------------------------------------------
    def _seed_args(self, who, seeds):
        """(kind, pointer, count, what must stay alive until the call returns) of the kinds of seeds that Geodesic and Access take"""
        if isinstance(seeds, str):
            if seeds != "border":
                raise DxvError(f"{who}: unknown seeds {seeds!r} (\"border\", an index array, an [N, N, N] array or a device tensor)")
            return GEO_SEEDS_BORDER, None, 0, None
        if hasattr(seeds, "data_ptr"):                                  # a device tensor: a mask read in place
            import torch
            if not seeds.is_cuda or seeds.dtype not in (torch.uint8, torch.bool) or not seeds.is_contiguous():
                raise DxvError(f"{who}: a seed tensor must be a contiguous uint8 or bool tensor on the device")
            n = self.stats()["grid_dim"]
            if seeds.numel() != n ** 3:
                raise DxvError(f"{who}: the seed tensor has {seeds.numel()} elements, the grid has {n ** 3} voxels")
            torch.cuda.current_stream(seeds.device).synchronize()       # (its writer is ordered before the frame's stream reads it)
            return GEO_SEEDS_MASK, C.c_void_p(seeds.data_ptr()), 0, seeds
        a = np.asarray(seeds)
        if a.ndim == 3:
            a = np.flatnonzero(a)
        if a.size and (a.min() < 0 or a.max() > 0xFFFFFFFF):
            raise DxvError(f"{who}: a seed index is outside the grid")
        a = np.ascontiguousarray(a.reshape(-1), np.uint32)
        return GEO_SEEDS_LIST, a.ctypes.data_as(C.c_void_p) if a.size else None, int(a.size), a

    def Geodesic(self, of=COMP_SOLID, metric=GEO_CHAMFER, seeds="border", limit=0, sync=True, frameIndex=None):
        """The geodesic distance inside the selected frame's whole grid on the device (dxv_geodesic / dxv_geodesic_async; include/dxv.h has the
        rule): per member voxel -- of = COMP_SOLID the non-zero voxels, COMP_EMPTY the zero ones -- the length of the shortest path of member
        voxels to the nearest seed, GEO_FACES over the 6 face neighbours at weight 1, GEO_CHAMFER over the 26 neighbours at weights 3 / 4 / 5;
        GEO_NONE on the others, GEO_UNREACHED where no path exists or, with limit != 0, is longer than limit.  seeds: "border"; a 1-D array of
        voxel indices (iz * N + iy) * N + ix; an [N, N, N] bool / uint8 host array (its non-zero voxels, sent as indices); or a torch uint8 / bool
        tensor of N^3 elements on the frame's device (read in place, after the tensor's stream has been waited for).  The grid and the frame's
        other products stay as they are.  sync=True returns GeodesicField(); sync=False only enqueues one batch of rounds."""
        if frameIndex is not None:
            self.SetFrame(frameIndex)
        fn = self._lib.dxv_geodesic if sync else self._lib.dxv_geodesic_async
        kind, ptr, count, keep = self._seed_args("Geodesic", seeds)
        self._check(fn(self._ctx, int(of), int(metric), kind, ptr, count, int(limit)))
        del keep
        return self.GeodesicField() if sync else True

    def GeodesicField(self):
        """numpy copy uint32 [N, N, N] (z, y, x) of the selected frame's geodesic map (dxv_geodesic_download; synchronises the frame)."""
        return self._download("geodesic", np.uint32, "cube", speaks="dxv_geodesic_device_ptr")

    def geodesic_device_ptr(self):
        """Device pointer of the selected frame's geodesic map, 4 * N^3 bytes, for consumers on the GPU (exact after Sync)."""
        return self._pointer("dxv_geodesic_device_ptr")

    def GeodesicInfo(self):
        """{ms, rounds, seeds_used, reached, unreached, farthest, farthest_voxel} of the selected frame's last geodesic as of its last Sync
        (dxv_geodesic_info).  rounds may differ from run to run; nothing reached: farthest 0 at voxel 0xFFFFFFFF."""
        ms, rounds, far, voxel = C.c_float(), C.c_uint32(), C.c_uint32(), C.c_uint32()
        used, reached, unreached = C.c_uint64(), C.c_uint64(), C.c_uint64()
        self._check(self._lib.dxv_geodesic_info(self._ctx, C.byref(ms), C.byref(rounds), C.byref(used), C.byref(reached), C.byref(unreached), C.byref(far), C.byref(voxel)))
        return {"ms": ms.value, "rounds": rounds.value, "seeds_used": used.value, "reached": reached.value, "unreached": unreached.value, "farthest": far.value,
                "farthest_voxel": voxel.value}

    def geodesic_work_info(self):
        """{tiles_run, most_live_tiles, sparse_rounds} of the selected frame's last geodesic as of its last Sync (dxv_geodesic_work_info): the live
        8^3 tiles summed over its rounds, the most of one round, the rounds with fewer than 1024 live tiles.  They differ from run to run."""
        tiles, most, sparse = C.c_uint64(), C.c_uint32(), C.c_uint32()
        self._check(self._lib.dxv_geodesic_work_info(self._ctx, C.byref(tiles), C.byref(most), C.byref(sparse)))
        return {"tiles_run": tiles.value, "most_live_tiles": most.value, "sparse_rounds": sparse.value}

    def GeodesicPath(self, target):
        """uint32 voxel indices of a shortest path from target down to a seed of the selected frame's map (dxv_geodesic_path; synchronous): at every
        voxel the first neighbour, in order of increasing index, whose value plus the step's weight is the voxel's own."""
        length = C.c_uint32()
        self._check(self._lib.dxv_geodesic_path(self._ctx, int(target), None, 0, C.byref(length)))
        out = np.empty(length.value, np.uint32)
        self._check(self._lib.dxv_geodesic_path(self._ctx, int(target), out.ctypes.data_as(C.c_void_p), len(out), C.byref(length)))
        return out[:length.value]

    # ---- what can get in: the access radius and the intrusion map of the frame's grid ---------------------
    def Access(self, of=COMP_EMPTY, connectivity=26, capSq=4096, seeds="border", intrusion=True, sync=True, frameIndex=None):
        """The access radius inside the selected frame's whole grid on the device, and its intrusion map (dxv_access / dxv_access_async;
        include/dxv.h has the rule): per member voxel -- of = COMP_SOLID the non-zero voxels, COMP_EMPTY the zero ones -- A = the squared radius
        of the largest voxel-centred ball whose centre can travel from a seed to the voxel without leaving the members (steps over the 6 or the
        26 neighbours; R = min(D2, capSq) as in Thickness), and with intrusion=True I = the largest such ball that covers the voxel; 0 on
        the others and where nothing gets to; 2 <= capSq <= 4096.  seeds as in Geodesic.  The grid and the frame's other products stay as they
        are.  sync=True returns (AccessField(), IntrusionField() or None); sync=False only enqueues one batch of rounds -- the intrusion map
        is made where the frame is next synchronised, and a seed tensor is read on the frame's stream, as by Geodesic: with sync=False the
        caller keeps it alive and unchanged until the frame has been synchronised (a list is copied before the call returns)."""
        if frameIndex is not None:
            self.SetFrame(frameIndex)
        fn = self._lib.dxv_access if sync else self._lib.dxv_access_async
        kind, ptr, count, keep = self._seed_args("Access", seeds)
        self._check(fn(self._ctx, int(of), int(connectivity), int(capSq), kind, ptr, count, 1 if intrusion else 0))
        del keep
        return (self.AccessField(), self.IntrusionField() if intrusion else None) if sync else True

    def AccessField(self):
        """numpy copy uint32 [N, N, N] (z, y, x) of the selected frame's access map, squared radii (dxv_access_download; synchronises the frame)."""
        return self._download("access", np.uint32, "cube", speaks="dxv_access_device_ptr")

    def AccessHistogram(self):
        """numpy copy uint64 [capSq + 1] of the access map's histogram: bin v the voxels with A == v (dxv_access_histogram_download)."""
        return self._download("access_histogram", np.uint64, speaks="dxv_access_device_ptr")

    def IntrusionField(self):
        """numpy copy uint32 [N, N, N] (z, y, x) of the selected frame's intrusion map, squared radii (dxv_intrusion_download; synchronises the
        frame); an error for an Access made with intrusion=False.  thickness_voxels turns it into voxels."""
        return self._download("intrusion", np.uint32, "cube", speaks="dxv_intrusion_device_ptr")

    def IntrusionHistogram(self):
        """numpy copy uint64 [capSq + 1] of the intrusion map's histogram (dxv_intrusion_histogram_download); intrusion_curve reads it."""
        return self._download("intrusion_histogram", np.uint64, speaks="dxv_intrusion_device_ptr")

    def access_device_ptrs(self):
        """(access map, intrusion map or None) device pointers of the selected frame, 4 * N^3 bytes each, for consumers on the GPU (exact after Sync)."""
        return self._pointer("dxv_access_device_ptr"), self._lib.dxv_intrusion_device_ptr(self._ctx) if self._lib.dxv_intrusion_bytes(self._ctx) else None

    def AccessInfo(self):
        """{ms, rounds, seeds_used, reached, unreached, widest, widest_voxel} of the selected frame's last access as of its last Sync
        (dxv_access_info).  rounds may differ from run to run; nothing reached: widest 0 at voxel 0xFFFFFFFF."""
        ms, rounds, widest, voxel = C.c_float(), C.c_uint32(), C.c_uint32(), C.c_uint32()
        used, reached, unreached = C.c_uint64(), C.c_uint64(), C.c_uint64()
        self._check(self._lib.dxv_access_info(self._ctx, C.byref(ms), C.byref(rounds), C.byref(used), C.byref(reached), C.byref(unreached), C.byref(widest), C.byref(voxel)))
        return {"ms": ms.value, "rounds": rounds.value, "seeds_used": used.value, "reached": reached.value, "unreached": unreached.value, "widest": widest.value,
                "widest_voxel": voxel.value}

    def access_work_info(self):
        """{tiles_run, most_live_tiles, sparse_rounds} of the selected frame's last access as of its last Sync (dxv_access_work_info), as
        geodesic_work_info.  They differ from run to run."""
        tiles, most, sparse = C.c_uint64(), C.c_uint32(), C.c_uint32()
        self._check(self._lib.dxv_access_work_info(self._ctx, C.byref(tiles), C.byref(most), C.byref(sparse)))
        return {"tiles_run": tiles.value, "most_live_tiles": most.value, "sparse_rounds": sparse.value}

    # ---- what a straight line reaches: the line-of-sight map of the frame's grid -------------------------
    def Sight(self, of=COMP_EMPTY, directions=SIGHT_ALL, sync=True, frameIndex=None):
        """The line-of-sight map of the selected frame's whole grid on the device (dxv_sight / dxv_sight_async; include/dxv.h has the rule):
        per voxel a uint32 with bit sight_bit(dx, dy, dz) set when the voxel is a member (COMP_EMPTY / COMP_SOLID) and every voxel behind it
        against the direction, up to the grid's border, is one too -- a ray entering the grid in that direction reaches it through members
        only.  directions: a non-empty subset of SIGHT_ALL.  sync=True returns SightField(); sync=False only enqueues it."""
        if frameIndex is not None:
            self.SetFrame(frameIndex)
        fn = self._lib.dxv_sight if sync else self._lib.dxv_sight_async
        self._check(fn(self._ctx, int(of), int(directions)))
        return self.SightField() if sync else True

    def SightField(self):
        """numpy copy uint32 [N, N, N] (z, y, x) of the selected frame's line-of-sight map (dxv_sight_download; synchronises the frame)."""
        return self._download("sight", np.uint32, "cube", speaks="dxv_sight_device_ptr")

    def sight_device_ptr(self):
        """device pointer of the selected frame's line-of-sight map, 4 * N^3 bytes, for consumers on the GPU (exact after Sync)."""
        return self._pointer("dxv_sight_device_ptr")

    def SightTally(self):
        """{members, seen uint64 [27], neither uint64 [13], count uint64 [27]} of the selected frame's map (dxv_sight_tally_download;
        synchronises the frame): the members, those seen along each direction's bit, per axis asked for both ways those seen along neither
        of its directions, and count[k] those seen along exactly k of the requested directions.  sight_axes ranks the axes."""
        words = np.empty(68, np.uint64)
        self._check(self._lib.dxv_sight_tally_download(self._ctx, words.ctypes.data_as(C.c_void_p), words.nbytes))
        return {"members": int(words[0]), "seen": words[1:28].copy(), "neither": words[28:41].copy(), "count": words[41:68].copy()}

    def SightInfo(self):
        """{ms, of, directions} of the selected frame's last line-of-sight map as of its last Sync (dxv_sight_info)."""
        ms, of, directions = C.c_float(), C.c_int(), C.c_uint32()
        self._check(self._lib.dxv_sight_info(self._ctx, C.byref(ms), C.byref(of), C.byref(directions)))
        return {"ms": ms.value, "of": of.value, "directions": directions.value}

    def SightFill(self, directions, sync=True):
        """Edit the selected frame's grid in place from its current line-of-sight map (dxv_sight_fill / _async): every member of the map's
        kind that is seen along none of `directions` (a non-empty subset of the map's) changes kind -- empty becomes 1, solid becomes 0.  An
        axis' two bits fill the undercuts of that pull axis, one bit the support volume of a build direction.  Every product of the frame,
        this map included, is stale afterwards."""
        fn = self._lib.dxv_sight_fill if sync else self._lib.dxv_sight_fill_async
        self._check(fn(self._ctx, int(directions)))
        return True

    def SelectComponents(self, rule, arg=0, sync=True):
        """Edit the selected frame's grid in place from its current labels (dxv_components_select / _async): the voxels of every component
        that rule does not keep become 0 (labels of COMP_SOLID) or 1 (COMP_EMPTY).  SELECT_LARGEST keeps the component with the most voxels,
        SELECT_MIN_VOXELS those with voxels >= arg, SELECT_BORDER those that touch the grid's border.  The labels are stale afterwards."""
        fn = self._lib.dxv_components_select if sync else self._lib.dxv_components_select_async
        self._check(fn(self._ctx, int(rule), int(arg)))
        return True

    def select_info(self):
        """(kept, dropped, voxels_changed) of the selected frame's last SelectComponents as of its last Sync (dxv_components_select_info)."""
        kept, dropped, changed = C.c_uint32(), C.c_uint32(), C.c_uint64()
        self._check(self._lib.dxv_components_select_info(self._ctx, C.byref(kept), C.byref(dropped), C.byref(changed)))
        return kept.value, dropped.value, changed.value

    # ---- the exterior flood fill of the frame's grid -----------------------------------------------
    def Fill(self, what=FILL_SOLID, sync=True, frameIndex=None):
        """Flood the empty space of the selected frame's whole grid from the grid's border (6-connectivity) and replace the grid, in
        place, by what the flood did not reach (dxv_fill / dxv_fill_async): FILL_SOLID the walls and everything they enclose,
        FILL_INTERIOR the enclosed voxels alone.  Voxelize(N, MODE_SURFACE); Fill() is the solid of a mesh whose normals and
        watertightness cannot be trusted.  sync=False only enqueues it behind the frame's launch."""
        if frameIndex is not None:
            self.SetFrame(frameIndex)
        if what not in (FILL_SOLID, FILL_INTERIOR):
            raise DxvError(f"Fill: unknown kind {what!r} (FILL_SOLID = 0, FILL_INTERIOR = 1)")
        fn = self._lib.dxv_fill if sync else self._lib.dxv_fill_async
        self._check(fn(self._ctx, int(what)))
        return True

    def fill_info(self):
        """(ms, rounds) of the selected frame's last fill as of its last Sync (dxv_fill_info)."""
        ms, rounds = C.c_float(), C.c_uint32()
        self._check(self._lib.dxv_fill_info(self._ctx, C.byref(ms), C.byref(rounds)))
        return ms.value, rounds.value

    # ---- morphology of the frame's grid by the Euclidean ball ----------------------------------------
    def Morph(self, op, radiusSq, sync=True, frameIndex=None):
        """Grow or shrink the solid of the selected frame's whole grid by the ball { v : |v|^2 <= radiusSq } (1 .. 4096), in place, bytes 0 / 1
        (dxv_morph / dxv_morph_async; include/dxv.h has the rule): MORPH_DILATE, MORPH_ERODE, MORPH_OPEN = dilate(erode), MORPH_CLOSE =
        erode(dilate).  Voxels outside the grid do not exist.  Voxelize(N, MODE_SURFACE); Morph(MORPH_DILATE, r2); Fill(); Morph(MORPH_ERODE, r2)
        seals holes narrower than the ball.  sync=False only enqueues it behind whatever the frame's stream holds."""
        if frameIndex is not None:
            self.SetFrame(frameIndex)
        fn = self._lib.dxv_morph if sync else self._lib.dxv_morph_async
        self._check(fn(self._ctx, int(op), int(radiusSq)))
        return True

    def morph_info(self):
        """(ms, voxels_set, voxels_cleared) of the selected frame's last morph as of its last Sync (dxv_morph_info)."""
        ms, was_set, cleared = C.c_float(), C.c_uint64(), C.c_uint64()
        self._check(self._lib.dxv_morph_info(self._ctx, C.byref(ms), C.byref(was_set), C.byref(cleared)))
        return ms.value, was_set.value, cleared.value

    # ---- topology-preserving thinning of the frame's grid ---------------------------------------------
    def Thin(self, kind, max_iterations=0, sync=True, frameIndex=None):
        """Thin the solid of the selected frame's whole grid without changing its topology, in place, bytes 0 / 1 (dxv_thin / dxv_thin_async;
        include/dxv.h has the rule): THIN_CURVE leaves a curve skeleton, THIN_KERNEL the topological kernel (a voxel per blob, a ring per
        handle).  Voxels outside the grid are empty.  max_iterations=0: to the fixed point.  Voxelize(N, MODE_SURFACE); Fill(); Thin(THIN_CURVE)
        is the centre line of a mesh.  sync=False only enqueues one batch of iterations behind whatever the frame's stream holds."""
        if frameIndex is not None:
            self.SetFrame(frameIndex)
        fn = self._lib.dxv_thin if sync else self._lib.dxv_thin_async
        self._check(fn(self._ctx, int(kind), int(max_iterations)))
        return True

    def thin_info(self):
        """(ms, iterations, voxels_removed, converged) of the selected frame's last thin as of its last Sync (dxv_thin_info)."""
        ms, iterations, removed, converged = C.c_float(), C.c_uint32(), C.c_uint64(), C.c_int()
        self._check(self._lib.dxv_thin_info(self._ctx, C.byref(ms), C.byref(iterations), C.byref(removed), C.byref(converged)))
        return ms.value, iterations.value, removed.value, converged.value

    def grid_bytes(self):
        return self._lib.dxv_grid_bytes(self._ctx)

    # ---- plumbing ---------------------------------------------------------------------------
    def set_stream(self, hip_stream):
        self._check(self._lib.dxv_set_stream(self._ctx, C.c_void_p(hip_stream) if hip_stream else None))

    def set_option(self, key, value):
        self._check(self._lib.dxv_set_option(self._ctx, key.encode(), int(value)))

    def stats(self):
        s = Stats()
        self._check(self._lib.dxv_get_stats(self._ctx, C.byref(s)))
        return s.as_dict()

    def build_lists(self, parity=False, grid=0):
        """Build the candidate lists of the reference rule now (they then travel with scene_export); parity=True: the parity
        rule's row lists as well; grid: the grid size the scene will be launched at (the lists' map follows it)."""
        self._check(self._lib.dxv_build_lists_for_grid(self._ctx, int(grid)) if grid else self._lib.dxv_build_lists(self._ctx))
        if parity:
            self._check(self._lib.dxv_build_parity_lists(self._ctx))

    def scene_bytes(self):
        return self._lib.dxv_scene_bytes(self._ctx)

    def scene_export(self, device_ptr, nbytes):
        self._check(self._lib.dxv_scene_export(self._ctx, C.c_void_p(device_ptr), nbytes))

    def scene_import(self, device_ptr, nbytes):
        self._check(self._lib.dxv_scene_import(self._ctx, C.c_void_p(device_ptr), nbytes))

    def list_check(self, gridDim, z0=0, nz=None):
        """(accepted (ray, triangle) pairs, violations, [(voxel id, triangle slot), ...]) of dxv_debug_list_check over slices
        [z0, z0 + nz) (default: the whole grid)."""
        out = np.zeros(34, np.uint64)
        nz = gridDim - z0 if nz is None else nz
        self._check(self._lib.dxv_debug_list_check(self._ctx, int(gridDim), int(z0), int(nz), out.ctypes.data_as(C.c_void_p)))
        nv = int(min(out[1], 16))
        return int(out[0]), int(out[1]), [(int(out[2 + 2 * k]), int(out[3 + 2 * k])) for k in range(nv)]

    def class_check(self, gridDim, z0=0, nz=None):
        """(hits on classified triangles, disagreements with the predicate, all hits, [(voxel id, triangle slot), ...]) of
        dxv_debug_class_check."""
        out = np.zeros(34, np.uint64)
        nz = gridDim - z0 if nz is None else nz
        self._check(self._lib.dxv_debug_class_check(self._ctx, int(gridDim), int(z0), int(nz), out.ctypes.data_as(C.c_void_p)))
        nv = int(min(out[1], 15))
        return int(out[0]), int(out[1]), int(out[2]), [(int(out[3 + 2 * k]), int(out[4 + 2 * k])) for k in range(nv)]

    def plan_check(self):
        """dxv_debug_plan_check for the current frame's last launch (which went through a work queue): dict with live_voxels,
        live_bricks (bricks holding a live voxel, exact), queued_bricks, violations (live bricks that are not queued: must be 0),
        duplicates (bricks queued twice: must be 0) and the first violating brick words."""
        out = np.zeros(16, np.uint64)
        self._check(self._lib.dxv_debug_plan_check(self._ctx, out.ctypes.data_as(C.c_void_p)))
        return {"live_voxels": int(out[0]), "live_bricks": int(out[1]), "queued_bricks": int(out[2]), "violations": int(out[3]),
                "duplicates": int(out[4]), "first": [int(v) for v in out[5:5 + int(min(out[3], 11))]]}

    def queue_order(self):
        """dxv_debug_queue_order for the prepared queue the current frame's last launch ran: dict with items, shared_tiles (direction
        tiles in more than one queue's own share: must be 0), descents (neighbours of one class of one queue out of order: must be 0) and
        checksum (over queue, item number and brick word: two builds of one queue give the same)."""
        out = np.zeros(4, np.uint64)
        self._check(self._lib.dxv_debug_queue_order(self._ctx, out.ctypes.data_as(C.c_void_p)))
        return {"items": int(out[0]), "shared_tiles": int(out[1]), "descents": int(out[2]), "checksum": int(out[3])}

    def division_check(self, n_first, n_last):
        """dxv_debug_division_check: (voxel origins checked, origins where a set-up word differs from the IEEE quotient's, first ids) over
        every even grid size in [n_first, n_last]."""
        out = np.zeros(8, np.uint64)
        self._check(self._lib.dxv_debug_division_check(self._ctx, int(n_first), int(n_last), out.ctypes.data_as(C.c_void_p)))
        return int(out[0]), int(out[1]), [int(v) for v in out[2:2 + int(min(out[1], 6))]]

    def far_check(self, gridDim, z0=0, nz=None, lists_mip=False):
        """dxv_debug_far_check: dict with bricks, dead_bricks (the brick test of the brick-box launches calls them dead), rays_walked
        (their rays, walked through the LBVH), violations (rays among them that hit something: must be 0) and the first voxel ids."""
        out = np.zeros(12, np.uint64)
        nz = gridDim - z0 if nz is None else nz
        self._check(self._lib.dxv_debug_far_check(self._ctx, int(gridDim), int(z0), int(nz), int(bool(lists_mip)), out.ctypes.data_as(C.c_void_p)))
        return {"bricks": int(out[0]), "dead_bricks": int(out[1]), "rays_walked": int(out[2]), "violations": int(out[3]),
                "first": [int(v) for v in out[4:4 + int(min(out[3], 8))]]}

    def debug_scan(self, what, lanes, buf, items):
        """dxv_debug_scan: the grid operators' exclusive scan on the caller's numbers, in place in `buf` (a C-contiguous array, or None) --
        what = 0: items x lanes uint32 counts; what = 1: items x lanes uint64 sums, then `lanes` words for the totals and one guard word.
        Returns the `lanes` totals."""
        totals = (C.c_uint64 * 2)()
        self._check(self._lib.dxv_debug_scan(self._ctx, int(what), int(lanes), None if buf is None else buf.ctypes.data_as(C.c_void_p), int(items), totals))
        return [int(totals[k]) for k in range(min(int(lanes), 2))]

    def trim(self):
        self._check(self._lib.dxv_trim(self._ctx))

    def debug(self, what):
        st = self.stats()
        T = st["num_tris"]
        shapes = {DBG_SORTED_KEYS: ((T,), np.uint64), DBG_NODES: ((st["num_nodes"], 16), np.uint32),
                  DBG_TRI_POS: ((T, 12), np.float32), DBG_TRI_NRM: ((T, 12), np.float32),
                  DBG_PARENTS: ((2 * T - 1,), np.uint32), DBG_NODES32: ((st["num_nodes"], 8), np.uint32),
                  DBG_NODES64: ((st["num_nodes"], 16), np.uint32),
                  DBG_LIST_CELLS: ((6 * st["list_res"] ** 2, 4), np.uint32), DBG_LIST_ENTRIES: ((st["list_entries"], 4), np.uint32),
                  DBG_LIST_STARTS: ((6 * st["list_res"] ** 2,), np.uint32), DBG_LIST_START_CELLS: ((6 * st["list_res"] ** 2, 4), np.uint32),
                  DBG_LIST_MIP: ((sum(6 * (st["list_res"] >> l) ** 2 for l in range(max(st["list_res"], 1).bit_length())),), np.uint16),
                  DBG_BRICK_EMPTY: (((st["grid_dim"] + 7) // 8,) * 3, np.uint8), DBG_BRICK_SUMMARY: (((st["grid_dim"] + 7) // 8,) * 3, np.uint8)}
        shape, dt = shapes[what]
        out = np.empty(shape, dt)
        self._check(self._lib.dxv_debug_download(self._ctx, what, out.ctypes.data_as(C.c_void_p), out.nbytes))
        return out
