"""The lists' per-record lateral bound (dxv_dirmap.h: dm_lateral_pad, option lateralpad) on the device: grids byte-equal to the oracle's
and between lateralpad 0 and 1 through every launch path (prepared, unprepared, kept queue, brick box), with and without the start
table, the texel image on once; no more list entries with the bound than without, strictly fewer on bunny; the exhaustive list check
and the class check report nothing; the device's entry count is the host replica's; export -> import gives the same grid; and flipping
the option drops the prepared queue."""
import numpy as np
import pytest

import edge_centre_cases as cases
from lateral_pad_cases import grazing_fan, sliver_mesh
from start_table_cases import HostLists

pytestmark = pytest.mark.gpu

SIDES = (32, 48, 64)            # 48: N % 16 == 0, no power of two, below the map


@pytest.fixture(scope="module")
def dxv(dxvlib):
    import dxrvoxelizer_amd
    return dxrvoxelizer_amd


@pytest.fixture(scope="module")
def wanted(orc, bunny):
    """name -> (vb, ib, {N: the oracle's grid}): computed once, never written to"""
    rng = np.random.default_rng(20261020)
    meshes = dict(cases.meshes(bunny))
    meshes["slivers"] = sliver_mesh(rng)
    meshes["grazing fan"] = grazing_fan(rng)
    out = {}
    for name, (vb, ib) in meshes.items():
        assert len(ib) // 3 <= 5000 or name == "bunny"
        sc = orc.Scene(vb, ib)
        out[name] = (vb, ib, {N: sc.voxelize(N) for N in ((64,) if name == "bunny" else SIDES)})
    return out


def every_path(v, N, want, what):
    def same(path):
        g, st = v.Grid(), v.stats()
        assert np.array_equal(g, want), what + (path, int((g != want).sum()))
        assert st["list_entries"] > 0, what + (path,)
        return st

    v.set_option("prepared", 1); v.set_option("plan", 2)
    v.PrepareLaunch(N)
    v.Voxelize(N)
    assert same("prepared")["plan_prepared"] == 1, what
    v.set_option("prepared", 0)
    v.Voxelize(N)
    st = same("unprepared")
    assert st["plan_prepared"] == 0 and st["plan_bricks"] > 0, what
    v.set_option("plan", 1)
    v.Voxelize(N); v.Voxelize(N)
    same("kept")
    v.set_option("plan", 0)
    v.Voxelize(N)
    assert same("brick box")["plan_bricks"] == 0, what
    v.set_option("plan", 2); v.set_option("prepared", 1)
    return st["list_entries"]


@pytest.mark.parametrize("name", ("octahedron", "snapped", "slivers", "grazing fan", "bunny"))
def test_grids_entries_and_checks(dxv, wanted, name):
    vb, ib, want = wanted[name]
    v = dxv.Voxelizer(0)
    try:
        v.set_option("lists", 2)
        for N in want:
            assert want[N].any()
            v.InitFromArrays(vb, ib, gridDim=N)
            entries, texels = {}, {}
            for lateral in (0, 1):
                v.set_option("lateralpad", lateral)
                for table in (0, 1):
                    v.set_option("starttable", table)
                    entries[lateral] = every_path(v, N, want[N], (name, N, "lateralpad", lateral, "starttable", table))
                v.EnableTexels(True)                                    # the texel image, once per setting: the same image
                v.Voxelize(N)
                assert np.array_equal(v.Grid(), want[N]), (name, N, lateral, "texels")
                texels[lateral] = v.Texels().copy()
                v.EnableTexels(False)
            assert np.array_equal(texels[0], texels[1]), (name, N)
            print(name, N, "entries without the bound", entries[0], "with", entries[1])
            assert entries[1] <= entries[0], (name, N, entries)
            if name == "bunny":
                assert entries[1] < entries[0], entries
            # (lateralpad is 1 here)
            accepted, violations, first = v.list_check(N)
            assert accepted > 0 and violations == 0, (name, N, accepted, violations, first)
            classified, wrong, hits, first = v.class_check(N)
            assert hits > 0 and wrong == 0, (name, N, classified, wrong, first)
            st = v.stats()
            h = HostLists(vb, ib, st["list_res"])
            try:
                assert st["list_entries"] == h.n == entries[1], (name, N, st["list_entries"], h.n)
            finally:
                h.close()
            v.set_option("starttable", 2)
    finally:
        v.close()


def test_round_trip_and_the_prepared_queue(dxv, wanted):
    import torch
    vb, ib, want = wanted["bunny"]
    N = 64
    v, w = dxv.Voxelizer(0), dxv.Voxelizer(0)
    try:
        v.set_option("lists", 2)
        v.InitFromArrays(vb, ib, gridDim=N)
        v.PrepareLaunch(N)
        v.Voxelize(N)
        st1 = v.stats()
        assert st1["plan_prepared"] == 1 and np.array_equal(v.Grid(), want[N])
        # flipping the option drops lists and prepared queue: the next launch builds lists again and finds no queue prepared for them
        v.set_option("lateralpad", 0)
        v.Voxelize(N)
        st0 = v.stats()
        assert st0["plan_prepared"] == 0 and st0["list_entries"] > st1["list_entries"] and np.array_equal(v.Grid(), want[N])
        v.PrepareLaunch(N)
        v.Voxelize(N)
        assert v.stats()["plan_prepared"] == 1 and np.array_equal(v.Grid(), want[N])
        v.set_option("lateralpad", 0)                                   # (the same value again: nothing is dropped)
        v.Voxelize(N)
        assert v.stats()["plan_prepared"] == 1
        v.set_option("lateralpad", 1)
        v.Voxelize(N)
        st = v.stats()
        assert st["plan_prepared"] == 0 and st["list_entries"] == st1["list_entries"] and np.array_equal(v.Grid(), want[N])
        # export -> import: the importing context voxelizes through the exporter's lists, whatever its own option says
        n = v.scene_bytes()
        blob = torch.empty(n, dtype=torch.uint8, device="cuda")
        v.scene_export(blob.data_ptr(), n)
        torch.cuda.synchronize()
        w.set_option("lists", 2)
        w.set_option("lateralpad", 0)
        w.scene_import(blob.data_ptr(), n)
        w.Voxelize(N)
        sw = w.stats()
        assert sw["list_res"] == st["list_res"] and sw["list_entries"] == st["list_entries"]
        assert np.array_equal(w.Grid(), want[N])
    finally:
        v.close(), w.close()
