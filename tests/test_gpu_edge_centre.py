"""The lists' edge word with cells counted from the texel's centre, on the device: the turned octahedron (slanted edges through every texel it
crosses), its lattice-snapped version and the golden bunny at 32^3 and 64^3 with the map forced to 16 and 64 texels, through the prepared
work queue (k_voxelize_listed), the queue built in the launch (k_voxelize_queue) and the brick-box path, image off and on -- every grid the
oracle's; dxv_debug_list_check and dxv_debug_class_check find no violation; an exported scene imports to the same grid; and a blob that
carries the version of the corner-based edge words is refused."""
import numpy as np
import pytest

import edge_centre_cases as cases

pytestmark = pytest.mark.gpu

OLD_SCENE_VERSION = 8                                                   # the last version whose edge words counted from the texel's corner


@pytest.fixture(scope="module")
def dxv(dxvlib):
    import dxrvoxelizer_amd
    return dxrvoxelizer_amd


@pytest.fixture(scope="module")
def wanted(orc, bunny):
    """(vb, ib, {N: the oracle's grid}) per mesh: computed once, never written to"""
    out = {}
    for name, (vb, ib) in cases.meshes(bunny).items():
        scene = orc.Scene(vb, ib)
        out[name] = (vb, ib, {N: scene.voxelize(N) for N in (32, 64)})
    return out


def lists_paths(v, N, want, what):
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
    st = same("queue")
    assert st["plan_prepared"] == 0 and st["plan_bricks"] > 0, what
    v.set_option("plan", 0)
    v.Voxelize(N)
    st = same("brick box")
    assert st["plan_bricks"] == 0, what
    v.set_option("plan", 2); v.set_option("prepared", 1)


@pytest.mark.parametrize("name", ("octahedron", "snapped", "bunny"))
def test_grids_checks_and_round_trip(dxv, wanted, name):
    import torch
    vb, ib, want = wanted[name]
    for R in (16, 64):
        v = dxv.Voxelizer(0)
        try:
            v.set_option("listres", R)
            v.set_option("lists", 2)
            for N in (32, 64):
                assert want[N].any()
                v.InitFromArrays(vb, ib, gridDim=N)
                for texels in (False, True):
                    v.EnableTexels(texels)
                    lists_paths(v, N, want[N], (name, R, N, "texels", texels))
                v.EnableTexels(False)
                assert v.stats()["list_res"] == R
                accepted, violations, first = v.list_check(N)
                assert accepted > 0 and violations == 0, (name, R, N, accepted, violations, first)
                classified, wrong, hits, first = v.class_check(N)
                assert hits > 0 and wrong == 0, (name, R, N, classified, wrong, first)
            # export -> import: the importing context voxelizes through the exporter's lists
            n = v.scene_bytes()
            blob = torch.empty(n, dtype=torch.uint8, device="cuda")
            v.scene_export(blob.data_ptr(), n)
            torch.cuda.synchronize()
            w = dxv.Voxelizer(0)
            try:
                w.set_option("lists", 2)
                w.scene_import(blob.data_ptr(), n)
                w.Voxelize(64)
                st = w.stats()
                assert st["list_res"] == R and st["list_entries"] == v.stats()["list_entries"]
                assert np.array_equal(w.Grid(), want[64]), (name, R, "imported")
            finally:
                w.close()
        finally:
            v.close()


def test_blob_of_the_corner_based_version_is_refused(dxv, wanted):
    import torch
    vb, ib, want = wanted["octahedron"]
    v, w = dxv.Voxelizer(0), dxv.Voxelizer(0)
    try:
        v.set_option("lists", 2)
        v.InitFromArrays(vb, ib, gridDim=32)
        n = v.scene_bytes()
        blob = torch.empty(n, dtype=torch.uint8, device="cuda")
        v.scene_export(blob.data_ptr(), n)
        torch.cuda.synchronize()
        header = blob[:8].cpu().numpy().view(np.uint32)
        assert header[0] == 0x53565844 and header[1] == OLD_SCENE_VERSION + 1
        old = blob.clone()
        old[4:8] = torch.from_numpy(np.array([OLD_SCENE_VERSION], np.uint32).view(np.uint8)).to(old.device)
        torch.cuda.synchronize()
        with pytest.raises(dxv.DxvError):
            w.scene_import(old.data_ptr(), n)
        w.set_option("lists", 2)
        w.scene_import(blob.data_ptr(), n)                              # ... and the same bytes with their own version are taken
        w.Voxelize(32)
        assert np.array_equal(w.Grid(), want[32])
    finally:
        v.close(), w.close()
