"""The surface modes on the GPU (include/dxv.h: DXV_MODE_SURFACE = 2, DXV_MODE_REFERENCE_SURFACE = 3): every grid equals the numpy
restatement of the rule (tests/surface_restated.py) or its committed hashes (tests/golden/surface.json), voxel for voxel; mode 3 equals
the reference rule's grid OR the surface.  Partitions, poisoned grids, mode changes on one frame, frames in flight, the deep-stack redo,
withdrawn lists, refitted and imported scenes, the texel image's refusal and the C++ mirror."""
import hashlib
import json
import os
import subprocess

import numpy as np
import pytest

from conftest import GOLD, ROOT
import surface_restated as sr
from dxrvoxelizer_amd.voxelizer import DBG_TRI_POS

pytestmark = pytest.mark.gpu

SURFACE, REFERENCE_SURFACE = 2, 3


@pytest.fixture(scope="module")
def dxv(dxvlib):
    import dxrvoxelizer_amd
    return dxrvoxelizer_amd


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def gold_mesh(name):
    d = np.load(os.path.join(GOLD, "meshes", name + ".npz"))
    return d["vb"], d["ib"]


_restated = {}


def restated(name, N, vb=None, ib=None):
    key = (name, N)
    if key not in _restated:
        if vb is None:
            vb, ib = gold_mesh(name)
        _restated[key] = sr.surface_of_mesh(vb, ib, N)
    return _restated[key]


def grid(v, N, mode, **kw):
    v.Voxelize(N, mode=mode, **kw)
    return v.Grid()


def first_diff(a, b):
    d = np.argwhere(a != b)
    return f"{len(d)} voxels differ, first (z, y, x) = {tuple(d[0]) if len(d) else None}"


def check(got, want, what):
    assert got.shape == want.shape, what
    assert np.array_equal(got, want), f"{what}: {first_diff(got, want)}"


# ---- 1, 2: whole grids against the restatement -------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["turingbowl", "bunny", "dragon"])
def test_assets_64(dxv, grids64, name):
    vb, ib = gold_mesh(name)
    v = dxv.Voxelizer(0)
    v.InitFromArrays(vb, ib)
    surf = restated(name, 64)
    check(grid(v, 64, SURFACE), surf, f"{name} mode 2")
    solid = np.unpackbits(grids64[f"{name}_64_reference"])[: 64 ** 3].reshape(64, 64, 64)
    check(grid(v, 64, REFERENCE_SURFACE), solid | surf, f"{name} mode 3")
    assert v.stats()["voxelize_ms"] > 0
    v.close()


def test_bunny_256_and_dragon_at_grids_that_do_not_fill_bricks(dxv, grids_json):
    vb, ib = gold_mesh("bunny")
    v = dxv.Voxelizer(0)
    v.InitFromArrays(vb, ib)
    solid = grid(v, 256, 0)
    assert sha(solid) == grids_json["bunny/256/reference"]["sha256"]
    surf = restated("bunny", 256)
    check(grid(v, 256, SURFACE), surf, "bunny 256 mode 2")
    check(grid(v, 256, REFERENCE_SURFACE), solid | surf, "bunny 256 mode 3")
    vb, ib = gold_mesh("dragon")
    v.InitFromArrays(vb, ib)
    for N in (2, 6, 30, 66, 130, 258):
        solid = grid(v, N, 0)
        surf = restated("dragon", N)
        check(grid(v, N, SURFACE), surf, f"dragon {N} mode 2")
        check(grid(v, N, REFERENCE_SURFACE), solid | surf, f"dragon {N} mode 3")
    v.close()


# ---- 3: the committed hashes (the large-triangle path at 1024^3) ------------------------------------------------------------
def fixture_mesh(name):
    from dxrvoxelizer_amd import meshes
    if name == "torus1m":
        return meshes.torus()
    if name == "dragon9":
        return meshes.trisect(*gold_mesh("dragon"))
    return getattr(meshes, name)()


@pytest.mark.parametrize("key", ["torus1m/512", "dragon9/512", "cube/1024", "tetrahedron/1024"])
def test_surface_json_configurations(dxv, key):
    with open(os.path.join(GOLD, "surface.json")) as fh:
        want = json.load(fh)[key]
    name, N = key.split("/")
    N = int(N)
    v = dxv.Voxelizer(0)
    v.InitFromArrays(*fixture_mesh(name))
    for mode, tag in ((SURFACE, "surface"), (REFERENCE_SURFACE, "reference_surface")):
        v.Voxelize(N, mode=mode)
        assert v.CountSolid() == want[tag]["count"], (key, tag)
        assert sha(v.Grid()) == want[tag]["sha256"], (key, tag)
    if name == "cube":
        # the cube's faces lie on the grid's outer voxel faces: the closed test marks that outermost layer and nothing else
        v.Voxelize(N, mode=SURFACE, z0=0, nz=2)
        g = v.Grid()
        assert g[0].all() and g[1, 1:-1, 1:-1].sum() == 0 and g[1, 0].all() and g[1, :, -1].all()
    v.close()


# ---- 4, 5: partitions and poison ------------------------------------------------------------------------------------------
def shares(N, world, zblock):
    for rank in range(world):
        z = [rank * zblock + (lz // zblock) * zblock * world + lz % zblock for lz in range(N // world)]
        yield rank, np.asarray(z)


@pytest.mark.parametrize("N", [64, 256])
def test_slabs_and_block_cyclic_shares_equal_the_whole_grid(dxv, N):
    vb, ib = gold_mesh("bunny")
    v = dxv.Voxelizer(0)
    v.InitFromArrays(vb, ib)
    for mode in (SURFACE, REFERENCE_SURFACE):
        whole = grid(v, N, mode)
        if mode == SURFACE:
            check(whole, restated("bunny", N), f"bunny {N} mode 2")
        for z0, nz in ((13, 9), (0, 1), (N - 5, 5)):
            check(grid(v, N, mode, z0=z0, nz=nz), whole[z0:z0 + nz], f"mode {mode} slab {z0}+{nz}")
        for zblock in (4, 8):
            for rank, zs in shares(N, 8, zblock):
                v.VoxelizeInterleaved(N, rank, 8, zblock, mode=mode)
                check(v.Grid(), whole[zs], f"mode {mode} share {rank}/8 zblock {zblock}")
    v.close()


def test_poisoned_grid_is_rewritten(dxv):
    import torch
    from dxrvoxelizer_amd.slabs import device_grid_tensor
    vb, ib = gold_mesh("dragon")
    v = dxv.Voxelizer(0)
    v.InitFromArrays(vb, ib)
    solid = grid(v, 64, 0)
    surf = restated("dragon", 64)
    for mode, want in ((SURFACE, surf), (REFERENCE_SURFACE, solid | surf), (SURFACE, surf)):
        v.Sync()
        device_grid_tensor(v, "cuda").fill_(0xAB)                        # (through dxv_grid_device_ptr)
        torch.cuda.synchronize()
        check(grid(v, 64, mode), want, f"mode {mode} after poison")
    v.close()


# ---- 6, 7: mode changes on one frame, frames in flight ------------------------------------------------------------------
@pytest.mark.parametrize("setup", ["defaults", "plan1", "prepared"])
def test_mode_changes_on_one_frame(dxv, setup):
    vb, ib = gold_mesh("bunny")
    N = 128
    v = dxv.Voxelizer(0)
    if setup == "plan1":
        v.set_option("plan", 1)
    v.InitFromArrays(vb, ib, gridDim=N if setup == "prepared" else 0)
    ref = dxv.Voxelizer(0)
    ref.InitFromArrays(vb, ib)
    solid = grid(ref, N, 0)
    ref.close()
    surf = restated("bunny", N)
    want = {0: solid, SURFACE: surf, REFERENCE_SURFACE: solid | surf}
    for step, mode in enumerate((0, 0, SURFACE, 0, REFERENCE_SURFACE, 0, 0, SURFACE, REFERENCE_SURFACE, 0)):
        check(grid(v, N, mode), want[mode], f"{setup}: step {step}, mode {mode}")
    v.close()


def test_three_frames_in_flight_with_different_modes(dxv):
    vb, ib = gold_mesh("dragon")
    N = 64
    v = dxv.Voxelizer(0)
    v.InitFromArrays(vb, ib)
    solid = grid(v, N, 0)
    surf = restated("dragon", N)
    want = {0: solid, SURFACE: surf, REFERENCE_SURFACE: solid | surf}
    for modes in ((SURFACE, 0, REFERENCE_SURFACE), (REFERENCE_SURFACE, SURFACE, 0), (0, REFERENCE_SURFACE, SURFACE)):
        for f, mode in enumerate(modes):
            v.Voxelize(N, mode=mode, sync=False, frameIndex=f)
        v.SyncAll()
        for f, mode in enumerate(modes):
            v.SetFrame(f)
            check(v.Grid(), want[mode], f"frame {f} mode {mode}")
    v.close()


# ---- 8: relaunches behind the surface pass ------------------------------------------------------------------------------------
def test_reference_surface_through_the_redo_pass(dxv):
    vb, ib = gold_mesh("dragon")
    ref = dxv.Voxelizer(0)
    ref.InitFromArrays(vb, ib)
    solid = grid(ref, 64, 0)
    ref.close()
    v = dxv.Voxelizer(0)
    v.set_option("lists", 0)
    v.InitFromArrays(vb, ib)
    v.set_option("stack", 8)
    check(grid(v, 64, REFERENCE_SURFACE), solid | restated("dragon", 64), "mode 3, stack 8")
    assert v.stats()["redo_rays"] > 0
    v.close()


def test_reference_surface_with_withdrawn_lists(dxv):
    # plates stacked along the x axis: the texels around it hold more entries than a list's count does, and the lists built for the
    # launch fail their deferred check: the frame is launched again through the tree -- and the shell again behind it
    K = 70000
    r = np.linspace(0.05, 1.0, K, dtype=np.float32)
    h = np.float32(0.04) * r
    one = np.stack([np.stack([r, -h, -h], 1), np.stack([r, h, -h], 1), np.stack([r, np.zeros_like(r), h], 1)], 1).reshape(-1, 3)
    pos = np.concatenate([one, one * np.array([-1, 1, 1], np.float32)])
    vb = np.ascontiguousarray(np.hstack([pos, np.tile(np.array([[1, 0, 0]], np.float32), (len(pos), 1))]), np.float32)
    ib = np.arange(len(pos), dtype=np.uint32)
    t = dxv.Voxelizer(0)
    t.set_option("lists", 0)
    t.InitDynamic(vb, ib)
    solid = grid(t, 64, 0)
    t.close()
    want = solid | sr.surface_of_mesh(vb, ib, 64)
    v = dxv.Voxelizer(0)
    v.set_option("lists", 2)
    v.InitDynamic(vb, ib)
    check(grid(v, 64, REFERENCE_SURFACE), want, "mode 3, lists withdrawn")
    st = v.stats()
    assert st["list_entries"] == 0 and st["list_ms"] > 0                   # (built, then withdrawn)
    v.InitDynamic(vb, ib)
    v.Voxelize(64, mode=REFERENCE_SURFACE, sync=False)
    v.SyncAll()
    check(v.Grid(), want, "mode 3 async, lists withdrawn")
    v.close()


# ---- 9, 10: refitted and imported scenes ----------------------------------------------------------------------------------------
def test_refitted_scene(dxv):
    vb, ib = gold_mesh("bunny")
    bound = sr.bound_of(vb)
    v = dxv.Voxelizer(0)
    v.InitDynamic(vb, ib)
    tp = v.debug(DBG_TRI_POS)                                              # the scene's normalised triangles ...
    order = tp[:, 3].view(np.uint32)                                       # (Morton order; w of vertex 0 = the triangle's index)
    want_tris = sr.normalised_tris(vb, ib)[order]
    assert np.array_equal(tp.reshape(-1, 3, 4)[:, :, :3], want_tris)       # ... are the restatement's normalisation
    for k in (1, 2):
        d = vb.copy()
        d[:, 0] += np.float32(0.08 * k) * np.sin(np.float32(7.0) * vb[:, 1])
        d[:, 2] *= np.float32(1.0 - 0.1 * k)
        v.UpdateVertices(d)                                                # refit: the bound of Init stays
        surf = sr.surface_of_mesh(d, ib, 96, bound=bound)
        check(grid(v, 96, SURFACE), surf, f"refit {k}, mode 2")
        solid = grid(v, 96, 0)
        check(grid(v, 96, REFERENCE_SURFACE), solid | surf, f"refit {k}, mode 3")
    v.close()


def test_imported_scene(dxv):
    import torch
    vb, ib = gold_mesh("dragon")
    a, b = dxv.Voxelizer(0), dxv.Voxelizer(0)
    a.InitFromArrays(vb, ib)
    n = a.scene_bytes()
    blob = torch.empty(n, dtype=torch.uint8, device="cuda")
    a.scene_export(blob.data_ptr(), n)
    torch.cuda.synchronize()
    b.scene_import(blob.data_ptr(), n)
    here = grid(a, 128, SURFACE)
    check(here, restated("dragon", 128), "exporting context")
    check(grid(b, 128, SURFACE), here, "importing context")
    check(grid(b, 128, REFERENCE_SURFACE), grid(a, 128, REFERENCE_SURFACE), "importing context, mode 3")
    a.close()
    b.close()


# ---- 11, 12: refusals, the C++ mirror -------------------------------------------------------------------------------------------
def test_texels_and_unknown_modes_are_refused(dxv):
    vb, ib = gold_mesh("bunny")
    v = dxv.Voxelizer(0)
    v.InitFromArrays(vb, ib)
    solid = grid(v, 64, 0)
    v.EnableTexels(True)
    for mode in (SURFACE, REFERENCE_SURFACE):
        with pytest.raises(dxv.DxvError) as e:
            v.Voxelize(64, mode=mode)
        assert "reference mode only" in str(e.value)
        check(grid(v, 64, 0), solid, f"mode 0 after a refused mode {mode}")
    v.EnableTexels(False)
    for mode in (4, -1):
        with pytest.raises(dxv.DxvError) as e:
            v.Voxelize(64, mode=mode)
        assert "unknown mode" in str(e.value)
    check(grid(v, 64, SURFACE), restated("bunny", 64), "mode 2 after the refusals")
    v.close()


def test_cpp_surface_modes(dxv, tmp_path):
    vb, ib = gold_mesh("dragon")
    np.ascontiguousarray(vb, np.float32).tofile(tmp_path / "vb.bin")
    np.ascontiguousarray(ib, np.uint32).tofile(tmp_path / "ib.bin")
    rocm = "/opt/rocm"
    exe = tmp_path / "surface_modes"
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-D__HIP_PLATFORM_AMD__", "-I" + os.path.join(rocm, "include"),
                           os.path.join(ROOT, "tests", "cpp", "surface_modes.cpp"), "-o", str(exe),
                           "-L" + os.path.join(ROOT, "dxrvoxelizer_amd"), "-l:libdxv.so", "-L" + os.path.join(rocm, "lib"), "-lamdhip64",
                           "-Wl,-rpath," + os.path.join(ROOT, "dxrvoxelizer_amd"), "-Wl,-rpath," + os.path.join(rocm, "lib")])
    r = subprocess.run([str(exe), str(tmp_path / "vb.bin"), str(tmp_path / "ib.bin"), "64", str(tmp_path / "surface.bin")],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    surface, shell = (int(x) for x in r.stdout.split())
    v = dxv.Voxelizer(0)
    v.InitFromArrays(vb, ib)
    v.Voxelize(64, mode=SURFACE)
    assert surface == v.CountSolid() == int(restated("dragon", 64).sum())
    v.Voxelize(64, mode=REFERENCE_SURFACE)
    assert shell == v.CountSolid()
    check(np.fromfile(tmp_path / "surface.bin", np.uint8).reshape(64, 64, 64), restated("dragon", 64), "C++ mirror")
    v.close()


# ---- a full work-item list (option surfaceitems: the list's capacity, lowered) -----------------------------------------------------
def test_full_work_item_list_gives_the_same_grids(dxv):
    """A large triangle whose work items do not all fit writes the ones that do and is walked whole as well; the reader never meets a
    slot nobody wrote in this launch.  Lowered caps make every case happen: none fit, some fit, a reservation runs past the end."""
    v = dxv.Voxelizer(0)
    with pytest.raises(dxv.DxvError):
        v.set_option("surfaceitems", (1 << 20) + 1)
    vb, ib = gold_mesh("dragon")
    v.InitFromArrays(vb, ib)
    want = restated("dragon", 258)
    for items in (1, 7, 300, 0):
        v.set_option("surfaceitems", items)
        check(grid(v, 258, SURFACE), want, f"dragon 258, surfaceitems {items}")
    solid = grid(v, 258, 0)
    v.set_option("surfaceitems", 3)
    check(grid(v, 258, REFERENCE_SURFACE), solid | want, "dragon 258 mode 3, surfaceitems 3")
    v.close()
    with open(os.path.join(GOLD, "surface.json")) as fh:
        fx = json.load(fh)["tetrahedron/1024"]
    t = dxv.Voxelizer(0)
    t.InitFromArrays(*fixture_mesh("tetrahedron"))                     # four faces of about 2,500 items each
    for items in (1, 700, 5000):
        t.set_option("surfaceitems", items)
        t.Voxelize(1024, mode=SURFACE)
        assert t.CountSolid() == fx["surface"]["count"], items
        assert sha(t.Grid()) == fx["surface"]["sha256"], items
    t.close()
