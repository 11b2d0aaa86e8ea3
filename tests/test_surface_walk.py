"""The surface pass's candidate enumeration (csrc/dxv_surface.h: tri_box, box_is_small, cols_setup, column_range -- the text the kernels of
surface.hip run, compiled for the CPU by tests/surface_host.py) held to the rule itself on hostile triangles (tests/surface_cases.py).
The truth is surface_restated.box_grid: the restated float32 test on EVERY voxel of the restated surface_box box -- no column walk, no
plane reasoning.  No GPU needed.

What this found: the column walk follows the exact plane, the float32 test of a triangle with a vertex of magnitude 10^4.5 or more does
not, and the walk lost voxels the test accepts (490 of 2,130 for the first listed triangle at N = 64).  Such triangles now walk their whole
box (kSurfaceFar); the walk without that limit stays selectable in the host check so that the cases can be seen to bite."""
import os
import subprocess

import numpy as np
import pytest

from conftest import GOLD, ROOT
import surface_cases as sc
import surface_host as sh
import surface_restated as sr

SIDES = (16, 32, 64, 100)
FAMILIES = ("on_face", "box_64_65", "slivers", "degenerates", "ties", "leaving", "far")
_cache = {}


def cases(N):
    if N not in _cache:
        fam = sc.families(N)
        if N > 64:                                               # (the truth costs N^3 tests for a triangle across the grid)
            fam["slivers"], fam["degenerates"] = fam["slivers"][::2], fam["degenerates"][::2]
            fam["far"] = np.concatenate([fam["far"][:-len(sc.LISTED)][::2], sc.listed()])
        _cache[N] = {name: (t, sr.box_grid(t, N)) for name, t in fam.items()}
    return _cache[N]


def differ(got, want):
    return f"{int((want & ~got).sum())} voxels missed, {int((got & ~want).sum())} too many"


def test_the_families_are_what_they_say():
    assert set(sc.families(16)) == set(FAMILIES)
    for N in SIDES:
        fam = sc.families(N)
        for name, t in fam.items():
            assert t.dtype == np.float32 and t.shape[1:] == (3, 3) and len(t) >= 15, (N, name)
            assert np.array_equal(t, sc.families(N)[name]), (N, name)                       # deterministic
        _, info = sh.surface(fam["on_face"], N)
        assert (info[:, 0] == sh.LARGE).all()                                                 # on a face: more than 64 candidates
        # (a side that is no power of two has no exact faces: centre and face are rounded, and the test may accept neither neighbour)
        assert (info[:, 2] > 0).all() or N & (N - 1)
        _, info = sh.surface(fam["box_64_65"], N)
        assert info[:, 0].tolist() == [sh.SMALL, sh.SMALL, sh.LARGE, sh.LARGE, sh.SMALL] * 3  # 64 voxels: the lane's own; 65: the walk
        assert info[info[:, 0] == sh.SMALL, 1].tolist() == [64] * 9
        mag = np.abs(fam["far"]).max((1, 2))
        for lo, hi in sc.BANDS:
            assert ((mag > 10 ** lo * 0.05) & (mag < 10 ** hi)).sum() >= 5
    # both neighbours of a face the plane lies on, one of them an ulp to either side -- also through the column walk
    for N in (16, 32, 64):
        t = sc.on_face(N)[3:6]                                                               # x = the face between voxels 2 and 3
        for k, want in enumerate(({2}, {2, 3}, {3})):
            g, info = sh.surface(t[k:k + 1], N)
            assert info[0, 0] == sh.LARGE and set(np.nonzero(g)[2]) == want, (N, k)


@pytest.mark.parametrize("N", SIDES)
def test_host_enumeration_equals_the_rule_on_the_whole_box(N):
    for name, (tris, want) in cases(N).items():
        assert want.any(), (N, name)
        for force in (False, True):
            got, info = sh.surface(tris, N, force_large=force)
            assert np.array_equal(got, want), f"N {N} {name} forced {force}: {differ(got, want)}"
            if force:
                assert not (info[:, 0] == sh.SMALL).any()
        # one triangle at a time: a neighbour cannot cover a miss
        for t in tris:
            counts = []
            want1 = sr.box_grid(t[None], N, counts) if name == "far" or N <= 32 else None
            for force in (False, True):
                got, info = sh.surface(t[None], N, force_large=force)
                if want1 is not None:
                    assert np.array_equal(got, want1), f"N {N} {name} {t.tolist()} forced {force}: {differ(got, want1)}"
                    assert int(info[0, 2]) == counts[0][1]
                    assert int(info[0, 1]) <= counts[0][0]                                    # candidates: within the box


def test_far_triangles_at_256():
    N = 256
    tris = np.concatenate([sc.top_band(N, 2), sc.listed(64)[:1]])
    for t in tris:
        want = sr.box_grid(t[None], N)
        for force in (False, True):
            got, _ = sh.surface(t[None], N, force_large=force)
            assert np.array_equal(got, want), f"{t.tolist()} forced {force}: {differ(got, want)}"


@pytest.mark.parametrize("N", SIDES)
def test_every_partition_equals_the_whole_grids_slices(N):
    for name, (tris, want) in cases(N).items():
        for z0, nz in ((13, 9), (0, 1), (N - 5, 5)):
            if z0 + nz <= N:
                got, _ = sh.surface(tris, N, z0=z0, nz=nz)
                assert np.array_equal(got, want[z0:z0 + nz]), f"N {N} {name} slab {z0}+{nz}: {differ(got, want[z0:z0 + nz])}"
        for world in (2, 8):
            for zblock in (4, 8):
                for rank, zs in sc.shares(N, world, zblock):
                    got, _ = sh.surface(tris, N, z0=rank * zblock, nz=len(zs), zblock=zblock, zperiod=zblock * world)
                    assert np.array_equal(got, want[zs]), f"N {N} {name} share {rank}/{world} zblock {zblock}: {differ(got, want[zs])}"


def test_the_far_vertex_cases_bite():
    """the walk without the far-vertex limit (the host check's switch; the kernels have none) loses voxels of every listed triangle"""
    lost = []
    for N, t in sc.LISTED:
        t = np.asarray(t, np.float32)[None]
        counts = []
        want = sr.box_grid(t, N, counts)
        old, info = sh.surface(t, N, old_walk=True)
        assert info[0, 0] == sh.LARGE
        assert not (old & ~want).any()
        lost.append(int((want & ~old).sum()))
        new, info = sh.surface(t, N)
        assert np.array_equal(new, want)
        assert np.abs(t).max() * N > sr.FAR_LIMIT and int(info[0, 1]) == counts[0][0]           # beyond the limit: the whole box
    assert all(n >= 1 for n in lost), lost
    assert lost[0] == 490 and int(sr.box_grid(np.asarray(sc.LISTED[0][1], np.float32)[None], 64).sum()) == 2130
    # the generated top band bites as well, the bands below 10^3.5 do not
    for N in (32, 64):
        tris, want = cases(N)["far"]
        old, _ = sh.surface(tris, N, old_walk=True)
        assert (want & ~old).any() and not (old & ~want).any()
        low = sc.far(N)[:20]
        old, _ = sh.surface(low, N, old_walk=True, force_large=True)
        assert np.array_equal(old, sr.box_grid(low, N))


@pytest.mark.parametrize("name", ["bunny", "dragon", "turingbowl"])
def test_in_range_meshes_keep_their_candidates(name):
    """a mesh inside its bound is below the limit: per triangle the same path and the same number of candidates with and without it"""
    d = np.load(os.path.join(GOLD, "meshes", name + ".npz"))
    tris = sr.normalised_tris(d["vb"], d["ib"])
    assert np.abs(tris).max() <= 1.0
    for force in (False, True):
        new, info_new = sh.surface(tris, 64, force_large=force)
        old, info_old = sh.surface(tris, 64, force_large=force, old_walk=True)
        assert np.array_equal(info_new, info_old)
        assert np.array_equal(new, old)
    assert np.array_equal(new, sr.surface_grid(tris, 64))
    # the limit itself: in range at every grid side the library takes
    assert all((1.0 + 2.0 / N) * N < sr.FAR_LIMIT for N in (2, 64, 2048))


@pytest.mark.parametrize("N", SIDES)
def test_the_restatements_own_walk_equals_the_whole_box(N):
    for name, (tris, want) in cases(N).items():
        got = sr.surface_grid(tris, N, large=1)
        assert np.array_equal(got, want), f"N {N} {name}: {differ(got, want)}"
    assert np.array_equal(sr.surface_grid(cases(N)["far"][0], N), cases(N)["far"][1])


def test_the_restated_limit_is_the_headers():
    with open(os.path.join(ROOT, "dxrvoxelizer_amd", "csrc", "dxv_surface.h")) as fh:
        assert "constexpr float kSurfaceFar = %.1ff;" % sr.FAR_LIMIT in fh.read()


def test_the_host_check_is_clean_under_the_sanitizers(tmp_path):
    """a program of its own (its own main, nothing loaded into Python) over the case families, written into a file for it"""
    exe, path = tmp_path / "surface_sanitize", tmp_path / "cases.bin"
    records = 0
    with open(path, "wb") as fh:
        for N in (16, 32, 64):
            for name, t in sc.families(N).items():
                fh.write(np.array([N, len(t)], np.uint32).tobytes() + np.ascontiguousarray(t, np.float32).tobytes())
                records += 1
        bad = np.array([[[np.nan, 0, 0], [0, 1, 0], [0, 0, 1]], [[np.inf, 0, 0], [0, 1, 0], [0, 0, 1]], [[3e38, -3e38, 3e38], [0, 1, 0], [-3e38, 0, 1]]], np.float32)
        fh.write(np.array([30, len(bad)], np.uint32).tobytes() + bad.tobytes())
        records += 1
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", str(exe),
                           os.path.join(ROOT, "tests", "cpp", "surface_sanitize_main.cpp")])
    r = subprocess.run([str(exe), str(path)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout[-1000:], r.stderr[-3000:])
    assert len(r.stdout.splitlines()) == records
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr
