"""What the operators on a frame's grid (include/dxv.h: dxv_distance*, dxv_mesh_distance*, dxv_isosurface*, dxv_octree*, dxv_components*,
dxv_measure*, dxv_thickness*, dxv_partition*, dxv_skeleton*, dxv_geodesic*, dxv_access*, dxv_intrusion*, dxv_fill*, dxv_morph*, dxv_thin*,
dxv_render_async) refuse, word for word: the WHOLE text of dxv_last_error against the sentence written out here, with ==.  A frame without a
grid, a slab, a product that was never made or went stale or was made without the part asked for, a wrong byte count, a NULL ms, a caller's
pointer the library cannot use -- and what is NOT said: a size never speaks (the measure's does), an empty table is NULL without a word.  One
cube at 16^3 throughout; every call under test returns before it enqueues anything, or works on 16^3.  And what a launch does to a fill, a thin, a
geodesic or an access of its frame that nobody has settled yet: it drops it; the verdict of an expansion it reads first."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N = 16
FIELD = 4 * N ** 3                                                      # bytes of a 16^3 field, of the labels, of a map
CAP_SQ = 17                                                             # of the thickness the tests make ...
HISTOGRAM = 8 * (CAP_SQ + 1)                                            # ... and the bytes of its histogram


@pytest.fixture(scope="module")
def dxv(dxvlib):
    import dxrvoxelizer_amd
    return dxrvoxelizer_amd


@pytest.fixture(scope="module")
def cube():
    from dxrvoxelizer_amd import meshes
    return meshes.cube()


@pytest.fixture
def v(dxv, cube):
    w = dxv.Voxelizer(0)
    try:
        w.InitFromArrays(*cube)
        yield w
    finally:
        w.close()


def last(v):
    return v._lib.dxv_last_error(v._ctx).decode()


def refused(v, rc, text):
    """the call failed (1, or NULL from an accessor that returns a pointer) and left exactly `text`"""
    assert rc in (1, None), (rc, text)
    assert last(v) == text


def operators(v):
    """every operator entry that wants the whole grid, enqueueing and blocking: (the name it speaks under, the call)"""
    lib, ctx = v._lib, v._ctx
    return [("dxv_distance", lambda: lib.dxv_distance_async(ctx, 1)), ("dxv_distance", lambda: lib.dxv_distance(ctx, 1)),
            ("dxv_octree", lambda: lib.dxv_octree_async(ctx)), ("dxv_octree", lambda: lib.dxv_octree(ctx)),
            ("dxv_octree_expand", lambda: lib.dxv_octree_expand_async(ctx, None, 0, 0)), ("dxv_octree_expand", lambda: lib.dxv_octree_expand(ctx, None, 0, 0)),
            ("dxv_components", lambda: lib.dxv_components_async(ctx, 0, 6)), ("dxv_components", lambda: lib.dxv_components(ctx, 0, 6)),
            ("dxv_fill", lambda: lib.dxv_fill_async(ctx, 0)), ("dxv_fill", lambda: lib.dxv_fill(ctx, 0)),
            ("dxv_morph", lambda: lib.dxv_morph_async(ctx, 0, 1)), ("dxv_morph", lambda: lib.dxv_morph(ctx, 0, 1)),
            ("dxv_thin", lambda: lib.dxv_thin_async(ctx, 0, 0)), ("dxv_thin", lambda: lib.dxv_thin(ctx, 0, 0)),
            ("dxv_thickness", lambda: lib.dxv_thickness_async(ctx, 0, CAP_SQ)), ("dxv_thickness", lambda: lib.dxv_thickness(ctx, 0, CAP_SQ)),
            ("dxv_geodesic", lambda: lib.dxv_geodesic_async(ctx, 0, 0, 0, None, 0, 0)), ("dxv_geodesic", lambda: lib.dxv_geodesic(ctx, 0, 0, 0, None, 0, 0)),
            ("dxv_measure", lambda: lib.dxv_measure_async(ctx)), ("dxv_measure", lambda: lib.dxv_measure(ctx)),
            ("dxv_partition", lambda: lib.dxv_partition_async(ctx, 0, CAP_SQ, 1)), ("dxv_partition", lambda: lib.dxv_partition(ctx, 0, CAP_SQ, 1)),
            ("dxv_skeleton", lambda: lib.dxv_skeleton_async(ctx, None)), ("dxv_skeleton", lambda: lib.dxv_skeleton(ctx, None)),
            ("dxv_access", lambda: lib.dxv_access_async(ctx, 0, 6, CAP_SQ, 0, None, 0, 1)), ("dxv_access", lambda: lib.dxv_access(ctx, 0, 6, CAP_SQ, 0, None, 0, 1))]


NO_GRID = {"dxv_distance": "dxv_distance: frame 1 has no grid yet (call dxv_voxelize first)",
           "dxv_octree": "dxv_octree: frame 1 has no grid yet (call dxv_voxelize first)",
           "dxv_octree_expand": "dxv_octree_expand: frame 1 has no grid yet (call dxv_voxelize first)",
           "dxv_components": "dxv_components: frame 1 has no grid yet (call dxv_voxelize first)",
           "dxv_fill": "dxv_fill: frame 1 has no grid yet (call dxv_voxelize first)",
           "dxv_morph": "dxv_morph: frame 1 has no grid yet (call dxv_voxelize first)",
           "dxv_thin": "dxv_thin: frame 1 has no grid yet (call dxv_voxelize first)",
           "dxv_thickness": "dxv_thickness: frame 1 has no grid yet (call dxv_voxelize first)",
           "dxv_geodesic": "dxv_geodesic: frame 1 has no grid yet (call dxv_voxelize first)",
           "dxv_measure": "dxv_measure: frame 1 has no grid yet (call dxv_voxelize first)",
           "dxv_partition": "dxv_partition: frame 1 has no grid yet (call dxv_voxelize first)",
           "dxv_skeleton": "dxv_skeleton: frame 1 has no grid yet (call dxv_voxelize first)",
           "dxv_access": "dxv_access: frame 1 has no grid yet (call dxv_voxelize first)"}
SLAB = {"dxv_distance": "dxv_distance: needs the whole grid of the frame's last launch (z0 = 0, nz = grid_dim), not a slab or a share",
        "dxv_octree": "dxv_octree: needs the whole grid of the frame's last launch (z0 = 0, nz = grid_dim), not a slab or a share",
        "dxv_octree_expand": "dxv_octree_expand: needs the whole grid of the frame's last launch (z0 = 0, nz = grid_dim), not a slab or a share",
        "dxv_components": "dxv_components: needs the whole grid of the frame's last launch (z0 = 0, nz = grid_dim), not a slab or a share",
        "dxv_fill": "dxv_fill: needs the whole grid of the frame's last launch (z0 = 0, nz = grid_dim), not a slab or a share",
        "dxv_morph": "dxv_morph: needs the whole grid of the frame's last launch (z0 = 0, nz = grid_dim), not a slab or a share",
        "dxv_thin": "dxv_thin: needs the whole grid of the frame's last launch (z0 = 0, nz = grid_dim), not a slab or a share",
        "dxv_thickness": "dxv_thickness: needs the whole grid of the frame's last launch (z0 = 0, nz = grid_dim), not a slab or a share",
        "dxv_geodesic": "dxv_geodesic: needs the whole grid of the frame's last launch (z0 = 0, nz = grid_dim), not a slab or a share",
        "dxv_measure": "dxv_measure: needs the whole grid of the frame's last launch (z0 = 0, nz = grid_dim), not a slab or a share",
        "dxv_partition": "dxv_partition: needs the whole grid of the frame's last launch (z0 = 0, nz = grid_dim), not a slab or a share",
        "dxv_skeleton": "dxv_skeleton: needs the whole grid of the frame's last launch (z0 = 0, nz = grid_dim), not a slab or a share",
        "dxv_access": "dxv_access: needs the whole grid of the frame's last launch (z0 = 0, nz = grid_dim), not a slab or a share"}


def test_a_frame_without_a_grid(v):
    lib, ctx = v._lib, v._ctx
    v.Voxelize(N)                                                       # frame 0 has one: the refusals below are frame 1's own
    v.SetFrame(1)
    for who, call in operators(v):
        refused(v, call(), NO_GRID[who])
    for fn in (lib.dxv_mesh_distance_async, lib.dxv_mesh_distance):
        refused(v, fn(ctx, 0, 0, 0), "dxv_mesh_distance: frame 1 has no grid yet (call dxv_voxelize first)")
    v.SetFrame(0)
    assert lib.dxv_octree(ctx) == 0                                     # ... and frame 0 is served


def test_a_slab_and_a_share(v, dxv):
    from dxrvoxelizer_amd import camera
    lib, ctx = v._lib, v._ctx
    v.Voxelize(N, z0=0, nz=8)
    slab = v.Grid()
    for who, call in operators(v):
        refused(v, call(), SLAB[who])
    eye, view_proj = camera.default_view_proj(8, 8)
    refused(v, lib.dxv_render_async(ctx, None, 32), "dxv_render_async: frame 0 has no ray-cast constants (call dxv_update_frame first)")
    v.UpdateFrame(0, eye, view_proj, 8, 8)
    refused(v, lib.dxv_render_async(ctx, None, 32),
            "dxv_render_async: needs the whole grid of the frame's last launch (z0 = 0, nz = grid_dim), not a slab or a share")
    # a slab's mesh distance field is made, and is no field to extract from
    assert lib.dxv_mesh_distance(ctx, 0, 0, 0) == 0
    refused(v, lib.dxv_isosurface(ctx, 0, 0.0, 0), "dxv_isosurface: the frame's mesh distance field is a slab's (8 of 16 slices); needs the field of the whole grid")
    assert np.array_equal(v.Grid(), slab)
    v.VoxelizeInterleaved(N, 0, 2, 4)
    for who, call in operators(v):
        refused(v, call(), SLAB[who])
    for fn in (lib.dxv_mesh_distance_async, lib.dxv_mesh_distance):
        refused(v, fn(ctx, 0, 0, 0), "dxv_mesh_distance: the frame's last launch was an interleaved share; needs the whole grid or a contiguous slab")


def accessors(v):
    """every accessor of a product by family: (its name, the call); downloads are given the right byte count where it is known here"""
    lib, ctx = v._lib, v._ctx
    buf = np.empty(FIELD, np.uint8)
    p = buf.ctypes.data_as(C.c_void_p)
    return {
        "distance": [("dxv_distance_device_ptr", lambda: lib.dxv_distance_device_ptr(ctx)),
                     ("dxv_distance_download", lambda: lib.dxv_distance_download(ctx, p, FIELD))],
        "mesh distance": [("dxv_mesh_distance_device_ptr", lambda: lib.dxv_mesh_distance_device_ptr(ctx)),
                          ("dxv_mesh_distance_triangles_device_ptr", lambda: lib.dxv_mesh_distance_triangles_device_ptr(ctx)),
                          ("dxv_mesh_distance_download", lambda: lib.dxv_mesh_distance_download(ctx, p, FIELD)),
                          ("dxv_mesh_distance_triangles_download", lambda: lib.dxv_mesh_distance_triangles_download(ctx, p, FIELD))],
        "isosurface": [("dxv_isosurface_counts", lambda: lib.dxv_isosurface_counts(ctx, None, None)),
                       ("dxv_isosurface_vertices_device_ptr", lambda: lib.dxv_isosurface_vertices_device_ptr(ctx)),
                       ("dxv_isosurface_indices_device_ptr", lambda: lib.dxv_isosurface_indices_device_ptr(ctx)),
                       ("dxv_isosurface_vertices_download", lambda: lib.dxv_isosurface_vertices_download(ctx, p, 24)),
                       ("dxv_isosurface_indices_download", lambda: lib.dxv_isosurface_indices_download(ctx, p, 12))],
        "octree": [("dxv_octree_info", lambda: lib.dxv_octree_info(ctx, None, None, None)),
                   ("dxv_octree_device_ptr", lambda: lib.dxv_octree_device_ptr(ctx)),
                   ("dxv_octree_download", lambda: lib.dxv_octree_download(ctx, p, 8)),
                   ("dxv_octree_expand", lambda: lib.dxv_octree_expand_async(ctx, None, 0, 0)),
                   ("dxv_octree_expand", lambda: lib.dxv_octree_expand(ctx, None, 0, 0))],
        "components": [("dxv_components_info", lambda: lib.dxv_components_info(ctx, None, None, None)),
                       ("dxv_components_labels_device_ptr", lambda: lib.dxv_components_labels_device_ptr(ctx)),
                       ("dxv_components_table_device_ptr", lambda: lib.dxv_components_table_device_ptr(ctx)),
                       ("dxv_components_labels_download", lambda: lib.dxv_components_labels_download(ctx, p, FIELD)),
                       ("dxv_components_table_download", lambda: lib.dxv_components_table_download(ctx, p, 24)),
                       ("dxv_components_select", lambda: lib.dxv_components_select_async(ctx, 0, 0)),
                       ("dxv_components_select", lambda: lib.dxv_components_select(ctx, 0, 0))],
        # (dxv_measure_table_bytes is the one size that speaks: 0 and the message, which `refused` is given as None)
        "measure": [("dxv_measure_table_device_ptr", lambda: lib.dxv_measure_table_device_ptr(ctx)),
                    ("dxv_measure_table_bytes", lambda: lib.dxv_measure_table_bytes(ctx) or None),
                    ("dxv_measure_table_download", lambda: lib.dxv_measure_table_download(ctx, p, 96))],
        "thickness": [("dxv_thickness_device_ptr", lambda: lib.dxv_thickness_device_ptr(ctx)),
                      ("dxv_thickness_download", lambda: lib.dxv_thickness_download(ctx, p, FIELD)),
                      ("dxv_thickness_histogram_download", lambda: lib.dxv_thickness_histogram_download(ctx, p, HISTOGRAM))],
        "geodesic": [("dxv_geodesic_device_ptr", lambda: lib.dxv_geodesic_device_ptr(ctx)),
                     ("dxv_geodesic_download", lambda: lib.dxv_geodesic_download(ctx, p, FIELD)),
                     ("dxv_geodesic_info", lambda: lib.dxv_geodesic_info(ctx, None, None, None, None, None, None, None)),
                     ("dxv_geodesic_work_info", lambda: lib.dxv_geodesic_work_info(ctx, None, None, None)),
                     ("dxv_geodesic_path", lambda: lib.dxv_geodesic_path(ctx, 0, None, 0, C.byref(C.c_uint32())))],
        "partition": [("dxv_partition_labels_device_ptr", lambda: lib.dxv_partition_labels_device_ptr(ctx)),
                      ("dxv_partition_labels_download", lambda: lib.dxv_partition_labels_download(ctx, p, FIELD)),
                      ("dxv_partition_table_device_ptr", lambda: lib.dxv_partition_table_device_ptr(ctx)),
                      ("dxv_partition_table_download", lambda: lib.dxv_partition_table_download(ctx, p, 32)),
                      ("dxv_partition_throats_device_ptr", lambda: lib.dxv_partition_throats_device_ptr(ctx)),
                      ("dxv_partition_throats_download", lambda: lib.dxv_partition_throats_download(ctx, p, 20))],
        "skeleton": [("dxv_skeleton_labels_device_ptr", lambda: lib.dxv_skeleton_labels_device_ptr(ctx)),
                     ("dxv_skeleton_labels_download", lambda: lib.dxv_skeleton_labels_download(ctx, p, FIELD)),
                     ("dxv_skeleton_nodes_device_ptr", lambda: lib.dxv_skeleton_nodes_device_ptr(ctx)),
                     ("dxv_skeleton_nodes_download", lambda: lib.dxv_skeleton_nodes_download(ctx, p, 32)),
                     ("dxv_skeleton_branches_device_ptr", lambda: lib.dxv_skeleton_branches_device_ptr(ctx)),
                     ("dxv_skeleton_branches_download", lambda: lib.dxv_skeleton_branches_download(ctx, p, 48)),
                     ("dxv_skeleton_prune", lambda: lib.dxv_skeleton_prune_async(ctx, 0)),
                     ("dxv_skeleton_prune", lambda: lib.dxv_skeleton_prune(ctx, 0))],
        "access": [("dxv_access_device_ptr", lambda: lib.dxv_access_device_ptr(ctx)),
                   ("dxv_access_download", lambda: lib.dxv_access_download(ctx, p, FIELD)),
                   ("dxv_access_histogram_download", lambda: lib.dxv_access_histogram_download(ctx, p, HISTOGRAM)),
                   ("dxv_access_info", lambda: lib.dxv_access_info(ctx, None, None, None, None, None, None, None)),
                   ("dxv_access_work_info", lambda: lib.dxv_access_work_info(ctx, None, None, None))],
        "intrusion": [("dxv_intrusion_device_ptr", lambda: lib.dxv_intrusion_device_ptr(ctx)),
                      ("dxv_intrusion_download", lambda: lib.dxv_intrusion_download(ctx, p, FIELD)),
                      ("dxv_intrusion_histogram_download", lambda: lib.dxv_intrusion_histogram_download(ctx, p, HISTOGRAM))],
    }


NONE_YET = {"distance": "%s: frame 0 has no distance field yet (call dxv_distance first)",
            "mesh distance": "%s: frame 0 has no mesh distance field yet (call dxv_mesh_distance first)",
            "isosurface": "%s: frame 0 has no isosurface yet (call dxv_isosurface first)",
            "octree": "%s: frame 0 has no octree yet (call dxv_octree first)",
            "components": "%s: frame 0 has no components yet (call dxv_components first)",
            "measure": "%s: frame 0 has no measure yet (call dxv_measure first)",
            "thickness": "%s: frame 0 has no thickness map yet (call dxv_thickness first)",
            "geodesic": "%s: frame 0 has no geodesic map yet (call dxv_geodesic first)",
            "partition": "%s: frame 0 has no partition yet (call dxv_partition first)",
            "skeleton": "%s: frame 0 has no skeleton yet (call dxv_skeleton first)",
            "access": "%s: frame 0 has no access map yet (call dxv_access first)",
            "intrusion": "%s: frame 0 has no access map yet (call dxv_access first)"}
STALE = {"distance": "%s: frame 0 was launched again since its distance field was made: the field is stale",
         "mesh distance": "%s: frame 0 was launched or filled again since its mesh distance field was made: the field is stale",
         "isosurface": "%s: frame 0 was launched or filled again since its isosurface was made: the mesh is stale",
         "octree": "%s: frame 0 was launched, filled or expanded again since its octree was made: the tree is stale",
         "components": "%s: frame 0 was launched, filled, expanded or selected again since its components were labelled: labels and table are stale",
         "measure": "%s: frame 0 was launched, edited or labelled again since its components were measured: the measure is stale",
         "thickness": "%s: frame 0 was launched or edited again since its thickness map was made: map and histogram are stale",
         "geodesic": "%s: frame 0 was launched or edited again since its geodesic map was made: the map is stale",
         "partition": "%s: frame 0 was launched or edited again since its partition was made: labels, table and throats are stale",
         "skeleton": "%s: frame 0 was launched or edited again since its skeleton was made: labels and tables are stale",
         "access": "%s: frame 0 was launched or edited again since its access map was made: maps and histograms are stale",
         "intrusion": "%s: frame 0 was launched or edited again since its access map was made: maps and histograms are stale"}


def make_every_product(v):
    lib, ctx = v._lib, v._ctx
    assert lib.dxv_distance(ctx, 1) == 0
    assert lib.dxv_mesh_distance(ctx, 0, 0, 1) == 0
    assert lib.dxv_isosurface(ctx, 0, 0.0, 0) == 0
    assert lib.dxv_octree(ctx) == 0
    assert lib.dxv_components(ctx, 0, 6) == 0
    assert lib.dxv_measure(ctx) == 0
    assert lib.dxv_thickness(ctx, 0, CAP_SQ) == 0
    assert lib.dxv_geodesic(ctx, 0, 0, 0, None, 0, 0) == 0
    assert lib.dxv_partition(ctx, 0, CAP_SQ, 1) == 0
    assert lib.dxv_skeleton(ctx, None) == 0
    assert lib.dxv_access(ctx, 0, 6, CAP_SQ, 0, None, 0, 1) == 0


def silent_sizes(v):
    """every size that never speaks (all of them but the measure's)"""
    lib, ctx = v._lib, v._ctx
    return (lib.dxv_distance_bytes(ctx), lib.dxv_mesh_distance_bytes(ctx), lib.dxv_octree_bytes(ctx), lib.dxv_components_labels_bytes(ctx),
            lib.dxv_components_table_bytes(ctx), lib.dxv_thickness_bytes(ctx), lib.dxv_thickness_histogram_bytes(ctx), lib.dxv_geodesic_bytes(ctx),
            lib.dxv_partition_labels_bytes(ctx), lib.dxv_partition_table_bytes(ctx), lib.dxv_partition_throats_bytes(ctx),
            lib.dxv_skeleton_labels_bytes(ctx), lib.dxv_skeleton_nodes_bytes(ctx), lib.dxv_skeleton_branches_bytes(ctx),
            lib.dxv_access_bytes(ctx), lib.dxv_access_histogram_bytes(ctx), lib.dxv_intrusion_bytes(ctx), lib.dxv_intrusion_histogram_bytes(ctx))


def sizes(v):
    """[0 .. 7] distance .. geodesic, [8] the measure's, [9 .. 18] partition .. intrusion"""
    silent = silent_sizes(v)
    return silent[:8] + (v._lib.dxv_measure_table_bytes(v._ctx),) + silent[8:]


NO_SIZES = (0,) * 19


def test_products_that_were_never_made_and_products_gone_stale(v):
    lib, ctx = v._lib, v._ctx
    v.Voxelize(N)
    for family, calls in accessors(v).items():
        for who, call in calls:
            refused(v, call(), NONE_YET[family] % who)
    refused(v, lib.dxv_isosurface(ctx, 0, 0.0, 0), "dxv_isosurface: frame 0 has no mesh distance field yet (call dxv_mesh_distance first)")
    refused(v, lib.dxv_isosurface_async(ctx, 1, 0.0, 0), "dxv_isosurface: frame 0 has no distance field yet (call dxv_distance first)")
    for fn in (lib.dxv_measure_async, lib.dxv_measure):                 # a grid and no labels to measure
        refused(v, fn(ctx), "dxv_measure: frame 0 has no components yet (call dxv_components first)")
    assert sizes(v) == NO_SIZES
    make_every_product(v)
    got = sizes(v)
    assert got[:2] == (FIELD, FIELD) and got[2] >= 8 and got[3] == FIELD and got[4] % 24 == 0 and got[4] > 0
    assert got[5:8] == (FIELD, HISTOGRAM, FIELD) and got[8] == 96 * (got[4] // 24 + 1)
    assert got[9] == FIELD and got[10] % 32 == 0 and got[10] > 0 and got[11] % 20 == 0                 # partition: labels, table, throats
    assert got[12] == FIELD and got[13] % 32 == 0 and got[14] % 48 == 0 and got[13] + got[14] > 0      # skeleton: labels, nodes, branches
    assert got[15:19] == (FIELD, HISTOGRAM, FIELD, HISTOGRAM)                                          # access and intrusion: map, histogram
    assert lib.dxv_distance_device_ptr(ctx) and lib.dxv_octree_info(ctx, None, None, None) == 0
    v.Voxelize(N)                                                       # launched again: every one of them is stale
    for family, calls in accessors(v).items():
        for who, call in calls:
            refused(v, call(), STALE[family] % who)
    refused(v, lib.dxv_isosurface(ctx, 0, 0.0, 0),
            "dxv_isosurface: frame 0 was launched or filled again since its mesh distance field was made: the field is stale")
    refused(v, lib.dxv_isosurface_async(ctx, 1, 0.0, 0),
            "dxv_isosurface: frame 0 was launched or filled again since its distance field was made: the field is stale")
    for fn in (lib.dxv_measure_async, lib.dxv_measure):
        refused(v, fn(ctx), "dxv_measure: frame 0 was launched, filled, expanded or selected again since its components were labelled: labels and table are stale")
    assert sizes(v) == NO_SIZES
    make_every_product(v)                                               # ... and can be made again
    assert sizes(v) == got


def test_a_field_without_triangles_and_a_field_in_the_int32_format(v):
    lib, ctx = v._lib, v._ctx
    buf = np.empty(FIELD, np.uint8)
    v.Voxelize(N)
    assert lib.dxv_mesh_distance(ctx, 0, 0, 0) == 0
    refused(v, lib.dxv_mesh_distance_triangles_device_ptr(ctx),
            "dxv_mesh_distance_triangles_device_ptr: frame 0's mesh distance field was made without triangles (want_triangles = 0)")
    refused(v, lib.dxv_mesh_distance_triangles_download(ctx, buf.ctypes.data_as(C.c_void_p), FIELD),
            "dxv_mesh_distance_triangles_download: frame 0's mesh distance field was made without triangles (want_triangles = 0)")
    assert lib.dxv_distance(ctx, 0) == 0
    refused(v, lib.dxv_isosurface(ctx, 1, 0.0, 0), "dxv_isosurface: the frame's distance field is in the int32 format; needs DXV_DIST_F32")


def test_a_partition_without_throats_and_an_access_without_intrusion(v):
    lib, ctx = v._lib, v._ctx
    buf = np.empty(FIELD, np.uint8)
    p = buf.ctypes.data_as(C.c_void_p)
    v.Voxelize(N)
    assert lib.dxv_partition(ctx, 0, CAP_SQ, 0) == 0
    refused(v, lib.dxv_partition_throats_device_ptr(ctx), "dxv_partition_throats_device_ptr: frame 0's partition was made without throats (want_throats = 0)")
    refused(v, lib.dxv_partition_throats_download(ctx, p, 0), "dxv_partition_throats_download: frame 0's partition was made without throats (want_throats = 0)")
    assert lib.dxv_partition_throats_bytes(ctx) == 0
    assert lib.dxv_partition_labels_device_ptr(ctx) and lib.dxv_partition_labels_bytes(ctx) == FIELD        # (the rest of it is handed out)
    assert lib.dxv_access(ctx, 0, 6, CAP_SQ, 0, None, 0, 0) == 0
    refused(v, lib.dxv_intrusion_device_ptr(ctx),
            "dxv_intrusion_device_ptr: the access map of frame 0 was made without its intrusion map (call dxv_access with want_intrusion != 0)")
    refused(v, lib.dxv_intrusion_download(ctx, p, FIELD),
            "dxv_intrusion_download: the access map of frame 0 was made without its intrusion map (call dxv_access with want_intrusion != 0)")
    refused(v, lib.dxv_intrusion_download(ctx, p, 0),
            "dxv_intrusion_download: the access map of frame 0 was made without its intrusion map (call dxv_access with want_intrusion != 0)")
    refused(v, lib.dxv_intrusion_histogram_download(ctx, p, HISTOGRAM),
            "dxv_intrusion_histogram_download: the access map of frame 0 was made without its intrusion map (call dxv_access with want_intrusion != 0)")
    assert lib.dxv_intrusion_bytes(ctx) == 0 and lib.dxv_intrusion_histogram_bytes(ctx) == 0
    assert lib.dxv_access_device_ptr(ctx) and lib.dxv_access_bytes(ctx) == FIELD and lib.dxv_access_histogram_bytes(ctx) == HISTOGRAM


def test_sizes_are_silent_except_the_one_that_speaks(v):
    lib, ctx = v._lib, v._ctx
    buf = np.empty(FIELD, np.uint8)
    p = buf.ctypes.data_as(C.c_void_p)
    v.Voxelize(N)
    # none yet
    said = "dxv_distance_download: frame 0 has no distance field yet (call dxv_distance first)"
    refused(v, lib.dxv_distance_download(ctx, p, FIELD), said)
    for size in silent_sizes(v):
        assert size == 0 and last(v) == said
    assert lib.dxv_measure_table_bytes(ctx) == 0
    assert last(v) == "dxv_measure_table_bytes: frame 0 has no measure yet (call dxv_measure first)"
    # stale
    make_every_product(v)
    v.Voxelize(N)
    said = "dxv_distance_download: frame 0 was launched again since its distance field was made: the field is stale"
    refused(v, lib.dxv_distance_download(ctx, p, FIELD), said)
    for size in silent_sizes(v):
        assert size == 0 and last(v) == said
    assert lib.dxv_measure_table_bytes(ctx) == 0
    assert last(v) == "dxv_measure_table_bytes: frame 0 was launched, edited or labelled again since its components were measured: the measure is stale"


def test_an_empty_table_is_null_without_a_word(v):
    from raycast_restated import write_grid
    lib, ctx = v._lib, v._ctx
    v.Voxelize(N)
    write_grid(v, np.zeros((N, N, N), np.uint8))
    assert lib.dxv_components(ctx, 0, 6) == 0, last(v)                  # (DXV_COMP_SOLID: no component)
    assert lib.dxv_skeleton(ctx, None) == 0, last(v)
    assert lib.dxv_partition(ctx, 0, CAP_SQ, 1) == 0, last(v)
    said = "dxv_distance_device_ptr: frame 0 has no distance field yet (call dxv_distance first)"
    refused(v, lib.dxv_distance_device_ptr(ctx), said)
    for ptr in (lib.dxv_components_table_device_ptr, lib.dxv_skeleton_nodes_device_ptr, lib.dxv_skeleton_branches_device_ptr,
                lib.dxv_partition_table_device_ptr, lib.dxv_partition_throats_device_ptr):
        assert ptr(ctx) is None and last(v) == said
    for size in (lib.dxv_components_table_bytes, lib.dxv_skeleton_nodes_bytes, lib.dxv_skeleton_branches_bytes, lib.dxv_partition_table_bytes,
                 lib.dxv_partition_throats_bytes):
        assert size(ctx) == 0
    for download in (lib.dxv_components_table_download, lib.dxv_skeleton_nodes_download, lib.dxv_skeleton_branches_download,
                     lib.dxv_partition_table_download, lib.dxv_partition_throats_download):
        assert download(ctx, None, 0) == 0, last(v)
    for ptr in (lib.dxv_components_labels_device_ptr, lib.dxv_skeleton_labels_device_ptr, lib.dxv_partition_labels_device_ptr):
        assert ptr(ctx)
    assert last(v) == said


def test_downloads_given_a_wrong_byte_count_or_no_buffer(v):
    lib, ctx = v._lib, v._ctx
    v.Voxelize(N)
    make_every_product(v)
    nv, nt, nodes, K = C.c_uint32(), C.c_uint32(), C.c_uint32(), C.c_uint32()
    regions, throats, skel_nodes, skel_branches = C.c_uint32(), C.c_uint32(), C.c_uint32(), C.c_uint32()
    assert lib.dxv_isosurface_counts(ctx, C.byref(nv), C.byref(nt)) == 0 and nv.value and nt.value
    assert lib.dxv_octree_info(ctx, None, C.byref(nodes), None) == 0 and nodes.value
    assert lib.dxv_components_info(ctx, C.byref(K), None, None) == 0 and K.value
    assert lib.dxv_partition_info(ctx, None, C.byref(regions), C.byref(throats), None) == 0 and regions.value
    assert lib.dxv_skeleton_info(ctx, None, C.byref(skel_nodes), C.byref(skel_branches), None, None, None) == 0 and skel_nodes.value + skel_branches.value
    # every download the checks above leave out: (its name, its call, what it asks for)
    others = (("dxv_measure_table_download", lib.dxv_measure_table_download, 96 * (K.value + 1)),
              ("dxv_thickness_download", lib.dxv_thickness_download, FIELD), ("dxv_thickness_histogram_download", lib.dxv_thickness_histogram_download, HISTOGRAM),
              ("dxv_geodesic_download", lib.dxv_geodesic_download, FIELD),
              ("dxv_partition_labels_download", lib.dxv_partition_labels_download, FIELD),
              ("dxv_partition_table_download", lib.dxv_partition_table_download, 32 * regions.value),
              ("dxv_partition_throats_download", lib.dxv_partition_throats_download, 20 * throats.value),
              ("dxv_skeleton_labels_download", lib.dxv_skeleton_labels_download, FIELD),
              ("dxv_skeleton_nodes_download", lib.dxv_skeleton_nodes_download, 32 * skel_nodes.value),
              ("dxv_skeleton_branches_download", lib.dxv_skeleton_branches_download, 48 * skel_branches.value),
              ("dxv_access_download", lib.dxv_access_download, FIELD), ("dxv_access_histogram_download", lib.dxv_access_histogram_download, HISTOGRAM),
              ("dxv_intrusion_download", lib.dxv_intrusion_download, FIELD), ("dxv_intrusion_histogram_download", lib.dxv_intrusion_histogram_download, HISTOGRAM))
    buf = np.empty(max(FIELD, 24 * nv.value, 12 * nt.value, 8 * nodes.value, 24 * K.value, max(want for _, _, want in others)) + 8, np.uint8)
    p = buf.ctypes.data_as(C.c_void_p)
    refused(v, lib.dxv_distance_download(ctx, p, 16385), "dxv_distance_download: expected 16384 bytes, got 16385")
    refused(v, lib.dxv_distance_download(ctx, None, 16384), "dxv_distance_download: expected 16384 bytes, got 16384")
    refused(v, lib.dxv_mesh_distance_download(ctx, p, 16380), "dxv_mesh_distance_download: expected 16384 bytes, got 16380")
    refused(v, lib.dxv_mesh_distance_download(ctx, None, 16384), "dxv_mesh_distance_download: expected 16384 bytes, got 16384")
    refused(v, lib.dxv_mesh_distance_triangles_download(ctx, p, 0), "dxv_mesh_distance_triangles_download: expected 16384 bytes, got 0")
    refused(v, lib.dxv_mesh_distance_triangles_download(ctx, None, 16384), "dxv_mesh_distance_triangles_download: expected 16384 bytes, got 16384")
    want = 24 * nv.value
    refused(v, lib.dxv_isosurface_vertices_download(ctx, p, want + 24), f"dxv_isosurface_vertices_download: expected {want} bytes, got {want + 24}")
    refused(v, lib.dxv_isosurface_vertices_download(ctx, None, want), f"dxv_isosurface_vertices_download: expected {want} bytes, got {want}")
    want = 12 * nt.value
    refused(v, lib.dxv_isosurface_indices_download(ctx, p, want - 12), f"dxv_isosurface_indices_download: expected {want} bytes, got {want - 12}")
    refused(v, lib.dxv_isosurface_indices_download(ctx, None, want), f"dxv_isosurface_indices_download: expected {want} bytes, got {want}")
    want = 8 * nodes.value
    refused(v, lib.dxv_octree_download(ctx, p, want + 8), f"dxv_octree_download: expected {want} bytes, got {want + 8}")
    refused(v, lib.dxv_octree_download(ctx, None, want), f"dxv_octree_download: expected {want} bytes, got {want}")
    refused(v, lib.dxv_components_labels_download(ctx, p, 4096), "dxv_components_labels_download: expected 16384 bytes, got 4096")
    refused(v, lib.dxv_components_labels_download(ctx, None, 16384), "dxv_components_labels_download: expected 16384 bytes, got 16384")
    want = 24 * K.value
    refused(v, lib.dxv_components_table_download(ctx, p, want + 1), f"dxv_components_table_download: expected {want} bytes, got {want + 1}")
    refused(v, lib.dxv_components_table_download(ctx, None, want), f"dxv_components_table_download: expected {want} bytes, got {want}")
    for who, fn, want in others:
        refused(v, fn(ctx, p, want + 1), f"{who}: expected {want} bytes, got {want + 1}")
        if want:                                                       # (a table without records has nothing to copy: NULL with 0 is served, below)
            refused(v, fn(ctx, None, want), f"{who}: expected {want} bytes, got {want}")
        else:
            assert fn(ctx, None, 0) == 0, last(v)
    # the same calls with what they ask for
    for who, fn, want in others:
        assert fn(ctx, p, want) == 0, last(v)
    for fn, want in ((lib.dxv_distance_download, FIELD), (lib.dxv_mesh_distance_download, FIELD), (lib.dxv_mesh_distance_triangles_download, FIELD),
                     (lib.dxv_isosurface_vertices_download, 24 * nv.value), (lib.dxv_isosurface_indices_download, 12 * nt.value),
                     (lib.dxv_octree_download, 8 * nodes.value), (lib.dxv_components_labels_download, FIELD),
                     (lib.dxv_components_table_download, 24 * K.value)):
        assert fn(ctx, p, want) == 0, last(v)


def test_ms_getters_refuse_null(v):
    lib, ctx = v._lib, v._ctx
    refused(v, lib.dxv_distance_ms(ctx, None), "dxv_distance_ms: ms is NULL")
    refused(v, lib.dxv_mesh_distance_ms(ctx, None), "dxv_mesh_distance_ms: ms is NULL")
    refused(v, lib.dxv_isosurface_ms(ctx, None), "dxv_isosurface_ms: ms is NULL")
    refused(v, lib.dxv_octree_ms(ctx, None), "dxv_octree_ms: ms is NULL")
    refused(v, lib.dxv_components_ms(ctx, None), "dxv_components_ms: ms is NULL")
    ms = C.c_float(-1.0)
    for fn in (lib.dxv_distance_ms, lib.dxv_mesh_distance_ms, lib.dxv_isosurface_ms, lib.dxv_octree_ms, lib.dxv_components_ms):
        assert fn(ctx, C.byref(ms)) == 0 and ms.value == 0.0            # nothing was made yet


def room_behind(ptr):
    """bytes from ptr to the end of the device allocation it lies in (the allocation is the caching allocator's segment, not the tensor)"""
    import torch
    for seg in torch.cuda.memory_snapshot():
        if seg["address"] <= ptr < seg["address"] + seg["total_size"]:
            return seg["address"] + seg["total_size"] - ptr
    raise AssertionError("no segment of the allocator holds the pointer")


def test_render_async_refuses_a_target_it_cannot_use(v):
    import torch
    from dxrvoxelizer_amd import camera
    lib, ctx = v._lib, v._ctx
    v.Voxelize(N)
    grid = v.Grid()
    eye, view_proj = camera.default_view_proj(8, 8)
    v.UpdateFrame(0, eye, view_proj, 8, 8)
    small = torch.zeros(256, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    ptr = small.data_ptr()
    assert ptr % 4 == 0
    refused(v, lib.dxv_render_async(ctx, None, 32), "dxv_render_async: target (nil) with row pitch 32: need a 4-byte aligned pointer and a pitch that is a multiple of 4 "
                                                    "and at least width * 4 = 32")
    refused(v, lib.dxv_render_async(ctx, C.c_void_p(ptr + 2), 32),
            f"dxv_render_async: target 0x{ptr + 2:x} with row pitch 32: need a 4-byte aligned pointer and a pitch that is a multiple of 4 "
            "and at least width * 4 = 32")
    refused(v, lib.dxv_render_async(ctx, C.c_void_p(ptr), 28),
            f"dxv_render_async: target 0x{ptr:x} with row pitch 28: need a 4-byte aligned pointer and a pitch that is a multiple of 4 "
            "and at least width * 4 = 32")
    pinned = torch.zeros(256, dtype=torch.uint8).pin_memory()
    refused(v, lib.dxv_render_async(ctx, C.c_void_p(pinned.data_ptr()), 32),
            f"dxv_render_async: 0x{pinned.data_ptr():x} is not device memory of device 0 (memory type 1, device 0)")
    host = np.zeros(256, np.uint8)
    refused(v, lib.dxv_render_async(ctx, host.ctypes.data_as(C.c_void_p), 32),
            f"dxv_render_async: 0x{host.ctypes.data:x} is not device memory of device 0 (memory type 0, device -2)")
    # 32 bytes in front of the tensor's end, rows far enough apart that the image runs past the end of the allocation
    near = ptr + 224
    pitch = 1 << 26
    need = 7 * pitch + 32
    has = room_behind(near)
    assert has < need
    refused(v, lib.dxv_render_async(ctx, C.c_void_p(near), pitch),
            f"dxv_render_async: 8 x 8 texels at pitch {pitch} need {need} bytes, the allocation behind 0x{near:x} has {has}")
    assert np.array_equal(v.Grid(), grid)
    assert lib.dxv_render_async(ctx, C.c_void_p(ptr), 32) == 0 and lib.dxv_sync(ctx) == 0        # the same call with what it asks for


def test_octree_expand_refuses_a_tree_it_cannot_use(v):
    import torch
    lib, ctx = v._lib, v._ctx
    v.Voxelize(N)
    grid = v.Grid()
    nodes, _ = v.Octree()
    n = len(nodes)
    tree = torch.from_numpy(np.ascontiguousarray(nodes, np.uint32).reshape(-1).view(np.int32)).cuda()
    torch.cuda.synchronize()
    ptr = tree.data_ptr()
    assert ptr % 4 == 0 and n >= 1                                     # (the cube fills this grid: its tree may be the root alone)

    def both(p, count, levels, text):
        for fn in (lib.dxv_octree_expand_async, lib.dxv_octree_expand):
            refused(v, fn(ctx, p, count, levels), text)

    both(C.c_void_p(ptr), 0, 4, "dxv_octree_expand: a tree of 0 nodes (the root is always there: nodes >= 1)")
    both(C.c_void_p(ptr), 0x80000000, 4, "dxv_octree_expand: a tree of 2147483648 nodes; at most 2147483647")
    both(C.c_void_p(ptr), n, 3, "dxv_octree_expand: a tree of 3 levels; the frame's grid of 16^3 voxels has 4")
    both(C.c_void_p(ptr), n, 5, "dxv_octree_expand: a tree of 5 levels; the frame's grid of 16^3 voxels has 4")
    both(C.c_void_p(ptr + 2), n, 4, f"dxv_octree_expand: nodes at 0x{ptr + 2:x}: need a 4-byte aligned pointer")
    pinned = torch.zeros(8 * n, dtype=torch.uint8).pin_memory()
    both(C.c_void_p(pinned.data_ptr()), n, 4, f"dxv_octree_expand: 0x{pinned.data_ptr():x} is not device memory of device 0 (memory type 1, device 0)")
    host = np.ascontiguousarray(nodes)
    both(host.ctypes.data_as(C.c_void_p), n, 4, f"dxv_octree_expand: 0x{host.ctypes.data:x} is not device memory of device 0 (memory type 0, device -2)")
    # the last node of the tensor as the first of a tree that is said to have as many as a tree can have
    near = ptr + 8 * (n - 1)
    has = room_behind(near)
    assert has < 8 * 0x7FFFFFFF
    both(C.c_void_p(near), 0x7FFFFFFF, 4, f"dxv_octree_expand: 2147483647 nodes need 17179869176 bytes, the allocation behind 0x{near:x} has {has}")
    assert np.array_equal(v.Grid(), grid)                              # nothing was written
    assert np.array_equal(v.OctreeNodes()[0], nodes)                   # ... and the frame's own tree is still current
    assert lib.dxv_octree_expand(ctx, C.c_void_p(ptr), n, 4) == 0      # the same call with what it asks for
    assert np.array_equal(v.Grid(), (grid != 0).astype(np.uint8))


def test_a_launch_drops_what_is_unsettled(v, dxv, cube):
    """a fill, a thin and a geodesic in batches of one round, each followed at once by a launch of the same frame: the launch's grid is a fresh
    context's, the operator's verdict is dropped with it, and the same operator afterwards gives what it gives in a fresh context"""
    lib, ctx = v._lib, v._ctx
    fresh = dxv.Voxelizer(0)
    try:
        fresh.InitFromArrays(*cube)
        fresh.Voxelize(N)
        launched = fresh.Grid()
        fresh.Fill()
        filled = fresh.Grid()
        fresh.Voxelize(N)
        fresh.Thin(dxv.THIN_CURVE)
        thinned, thinned_info = fresh.Grid(), fresh.thin_info()[1:]
        fresh.Voxelize(N)
        geodesic = fresh.Geodesic(dxv.COMP_SOLID, dxv.GEO_CHAMFER, "border")
    finally:
        fresh.close()
    try:
        for key in ("fillrounds", "thinrounds", "georounds"):
            v.set_option(key, 1)
        v.Voxelize(N)
        # fill
        assert lib.dxv_fill_async(ctx, 0) == 0
        v.Voxelize(N)
        assert np.array_equal(v.Grid(), launched)
        assert lib.dxv_fill(ctx, 0) == 0, last(v)
        assert np.array_equal(v.Grid(), filled)
        # thin
        v.Voxelize(N)
        assert lib.dxv_thin_async(ctx, 0, 0) == 0
        v.Voxelize(N)
        assert np.array_equal(v.Grid(), launched)
        assert v.thin_info()[3] == 0
        assert lib.dxv_thin(ctx, 0, 0) == 0, last(v)
        assert np.array_equal(v.Grid(), thinned) and v.thin_info()[1:] == thinned_info and thinned_info[2] == 1
        # geodesic
        v.Voxelize(N)
        assert lib.dxv_geodesic_async(ctx, 0, 1, 0, None, 0, 0) == 0
        v.Voxelize(N)
        assert np.array_equal(v.Grid(), launched)
        refused(v, lib.dxv_geodesic_info(ctx, None, None, None, None, None, None, None),
                "dxv_geodesic_info: frame 0 was launched or edited again since its geodesic map was made: the map is stale")
        assert lib.dxv_geodesic(ctx, 0, 1, 0, None, 0, 0) == 0, last(v)
        assert np.array_equal(v.GeodesicField(), geodesic)
        assert np.array_equal(v.Grid(), launched)                      # (a geodesic only reads the grid)
    finally:
        for key in ("fillrounds", "thinrounds", "georounds"):
            v.set_option(key, 0)


def test_a_launch_drops_an_unsettled_access(v, dxv, cube):
    """an access in batches of one round with its intrusion map, followed at once by a launch of the same frame: the launch's grid is a fresh
    context's, maps, histograms and tally are dropped with the batches nobody has read, and the same access afterwards gives what it gives in a
    fresh context"""
    lib, ctx = v._lib, v._ctx
    tally = ("seeds_used", "reached", "unreached", "widest", "widest_voxel")
    fresh = dxv.Voxelizer(0)
    try:
        fresh.InitFromArrays(*cube)
        fresh.Voxelize(N)
        launched = fresh.Grid()
        access, intrusion = fresh.Access(dxv.COMP_SOLID, 6, CAP_SQ, "border")
        histograms = fresh.AccessHistogram(), fresh.IntrusionHistogram()
        info = fresh.AccessInfo()
        assert access.any() and intrusion.any() and info["reached"] > 0
    finally:
        fresh.close()
    try:
        v.set_option("accessrounds", 1)
        v.Voxelize(N)
        assert lib.dxv_access_async(ctx, 0, 6, CAP_SQ, 0, None, 0, 1) == 0
        v.Voxelize(N)
        assert np.array_equal(v.Grid(), launched)
        refused(v, lib.dxv_access_info(ctx, None, None, None, None, None, None, None),
                "dxv_access_info: frame 0 was launched or edited again since its access map was made: maps and histograms are stale")
        refused(v, lib.dxv_intrusion_device_ptr(ctx), "dxv_intrusion_device_ptr: frame 0 was launched or edited again since its access map was made: maps and histograms are stale")
        assert lib.dxv_sync(ctx) == 0, last(v)                         # (nothing is left to settle)
        assert lib.dxv_access(ctx, 0, 6, CAP_SQ, 0, None, 0, 1) == 0, last(v)
        assert np.array_equal(v.AccessField(), access) and np.array_equal(v.IntrusionField(), intrusion)
        assert np.array_equal(v.AccessHistogram(), histograms[0]) and np.array_equal(v.IntrusionHistogram(), histograms[1])
        again = v.AccessInfo()
        assert {k: again[k] for k in tally} == {k: info[k] for k in tally}
        assert np.array_equal(v.Grid(), launched)                      # (an access only reads the grid)
    finally:
        v.set_option("accessrounds", 0)


def test_a_launch_behind_an_expansion_whose_verdict_nobody_has_read(v, dxv, cube):
    """an expansion from a caller's tree of another grid, followed at once by a launch of the same frame: the launch reads the verdict -- a
    well-formed tree has nothing to report --, its grid is the launch's and not the tree's, and no later synchronisation speaks of the tree"""
    from raycast_restated import write_grid
    from test_gpu_octree import as_device_words
    lib, ctx = v._lib, v._ctx
    v.Voxelize(N)
    launched = v.Grid()
    other = launched.copy()
    other[:N // 2] = 0
    other[N // 2:, :3, :3] = 1
    assert other.any() and not np.array_equal(other != 0, launched != 0)
    write_grid(v, other)
    nodes, _ = v.Octree()
    tree = as_device_words(nodes)
    v.Voxelize(N)
    assert lib.dxv_octree_expand_async(ctx, C.c_void_p(tree.data_ptr()), len(nodes), 4) == 0, last(v)
    v.Voxelize(N)
    assert np.array_equal(v.Grid(), launched)
    refused(v, lib.dxv_octree_info(ctx, None, None, None), "dxv_octree_info: frame 0 was launched, filled or expanded again since its octree was made: the tree is stale")
    assert lib.dxv_sync(ctx) == 0, last(v)
    assert lib.dxv_octree_expand(ctx, C.c_void_p(tree.data_ptr()), len(nodes), 4) == 0, last(v)      # the same call, read at once
    assert np.array_equal(v.Grid(), (other != 0).astype(np.uint8))
