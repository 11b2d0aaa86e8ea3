"""The surface pass on the GPU held to the rule on hostile triangles (tests/surface_cases.py): every device grid equals
surface_restated.box_grid -- the restated float32 test on every voxel of the restated surface_box box, no walk, no plane -- and the grid the
product's own enumeration makes on the CPU (tests/surface_host.py).

The scene: two unreferenced pin vertices at (-1, -1, -1) and (1, 1, 1) and the triangles.  It is built (InitDynamic) with placeholders
inside the pins, so its bound is exactly c = 0, w = 1, and then refitted (UpdateVertices) to the case's positions: a far vertex keeps that
bound, and the device's normalised triangle is the case's, bit for bit -- checked through debug(DBG_TRI_POS) before any grid is trusted.
One triangle per launch, so that a neighbour cannot cover a miss; then a whole family in one scene, through slabs, block-cyclic shares and a
lowered work-item list.  (At 32^3 the library takes world 8 only with blocks of 4 slices, grid_dim % (zblock * world) == 0; blocks of 8 run
with world 2.)"""
import numpy as np
import pytest

import surface_cases as sc
import surface_host as sh
import surface_restated as sr
from dxrvoxelizer_amd.voxelizer import DBG_TRI_POS

pytestmark = pytest.mark.gpu

SURFACE = 2
PINS = np.array([[-1, -1, -1, 0, 0, 1], [1, 1, 1, 0, 0, 1]], np.float32)
PARTS = (("slab", 13, 9), ("slab", 0, 1), ("slab", 27, 5), ("share", 8, 4), ("share", 2, 4), ("share", 2, 8))


@pytest.fixture(scope="module")
def dxv(dxvlib):
    import dxrvoxelizer_amd
    return dxrvoxelizer_amd


def vertex_buffer(tris):
    pos = np.asarray(tris, np.float32).reshape(-1, 3)
    vb = np.hstack([pos, np.tile(np.array([[0, 0, 1]], np.float32), (len(pos), 1))])
    return np.ascontiguousarray(np.concatenate([vb, PINS]), np.float32)


def scene(dxv, count):
    """count placeholder triangles inside the pins: the bound of the build is the cube [-1, 1]^3"""
    v = dxv.Voxelizer(0)
    place = np.tile(np.array([[[-0.5, -0.5, 0.0], [0.5, -0.5, 0.0], [0.0, 0.5, 0.0]]], np.float32), (count, 1, 1))
    v.InitDynamic(vertex_buffer(place), np.arange(3 * count, dtype=np.uint32))
    return v


def move(v, tris):
    """refit the scene to tris; the device's normalised triangles must be tris bit for bit.  Returns them in the device's order."""
    tris = np.ascontiguousarray(tris, np.float32).reshape(-1, 3, 3)
    v.UpdateVertices(vertex_buffer(tris))
    tp = v.debug(DBG_TRI_POS)
    order = tp[:, 3].view(np.uint32)
    got = np.ascontiguousarray(tp.reshape(-1, 3, 4)[:, :, :3])
    assert sorted(order.tolist()) == list(range(len(tris)))
    assert np.array_equal(got.view(np.uint32), tris[order].view(np.uint32)), "the device's triangles are not the case's"
    return tris[order]


@pytest.fixture(scope="module")
def expected():
    """per (N, family): the triangles, per triangle the whole-box truth and the host check's grid; computed once"""
    out = {}
    sets = {32: sc.picked(32), 30: {k: t for k, t in sc.picked(30).items() if k in ("on_face", "degenerates")},
            64: {"far": np.concatenate([sc.listed(), sc.top_band(64, 12)])}}
    for N, fams in sets.items():
        for name, tris in fams.items():
            want = [sr.box_grid(t[None], N) for t in tris]
            host = [sh.surface(t[None], N)[0] for t in tris]
            out[N, name] = (tris, want, host)
    return out


def differ(got, want):
    return f"{int((want & ~got).sum())} voxels missed, {int((got & ~want).sum())} too many"


def one_at_a_time(dxv, expected, N, name):
    tris, want, host = expected[N, name]
    v = scene(dxv, 1)
    hit = 0
    for t, w, h in zip(tris, want, host):
        move(v, t[None])
        v.Voxelize(N, mode=SURFACE)
        got = v.Grid()
        assert np.array_equal(got, w), f"N {N} {name} {t.tolist()}: {differ(got, w)}"
        assert np.array_equal(got, h), f"N {N} {name} {t.tolist()}: host check: {differ(got, h)}"
        hit += int(w.any())
    v.close()
    assert hit >= len(tris) // 2


@pytest.mark.parametrize("name", ["on_face", "box_64_65", "slivers", "degenerates", "ties", "leaving", "far"])
def test_one_triangle_per_launch_32(dxv, expected, name):
    one_at_a_time(dxv, expected, 32, name)


def test_far_triangles_one_per_launch_64(dxv, expected):
    one_at_a_time(dxv, expected, 64, "far")
    tris, want, _ = expected[64, "far"]
    assert int(want[0].sum()) == 2130                     # the listed triangle the walk lost 490 voxels of


@pytest.mark.parametrize("name", ["on_face", "degenerates"])
def test_one_triangle_per_launch_partial_bricks_30(dxv, expected, name):
    one_at_a_time(dxv, expected, 30, name)


@pytest.mark.parametrize("name", ["on_face", "box_64_65", "slivers", "degenerates", "ties", "leaving", "far"])
def test_a_whole_family_through_partitions_and_a_short_item_list(dxv, expected, name):
    N = 32
    tris, want, _ = expected[N, name]
    union = np.zeros((N, N, N), np.uint8)
    for w in want:
        union |= w
    v = scene(dxv, len(tris))
    ordered = move(v, tris)
    host, _ = sh.surface(ordered, N)
    assert np.array_equal(host, union), differ(host, union)
    for items in (0, 1, 3):
        v.set_option("surfaceitems", items)
        v.Voxelize(N, mode=SURFACE)
        got = v.Grid()
        assert np.array_equal(got, union), f"{name} surfaceitems {items}: {differ(got, union)}"
        for kind, a, b in PARTS:
            if kind == "slab":
                v.Voxelize(N, mode=SURFACE, z0=a, nz=b)
                got = v.Grid()
                assert np.array_equal(got, union[a:a + b]), f"{name} surfaceitems {items} slab {a}+{b}: {differ(got, union[a:a + b])}"
                assert np.array_equal(got, sh.surface(ordered, N, z0=a, nz=b)[0])
            else:
                for rank, zs in sc.shares(N, a, b):
                    v.VoxelizeInterleaved(N, rank, a, b, mode=SURFACE)
                    got = v.Grid()
                    assert np.array_equal(got, union[zs]), f"{name} surfaceitems {items} share {rank}/{a} zblock {b}: {differ(got, union[zs])}"
                    assert np.array_equal(got, sh.surface(ordered, N, z0=rank * b, nz=len(zs), zblock=b, zperiod=a * b)[0])
    v.close()
