"""MI355X-native solid voxelizer: the ray-traced occupancy hot path of StarsX/DXRVoxelizer.

Python here is plumbing (ctypes over the C-ABI of libdxv.so, torch.distributed for the one-off
scene broadcast); the product is the HIP library built from dxrvoxelizer_amd/csrc.
"""
from ._lib import DxvError, load_library, library_path  # noqa: F401
from .voxelizer import COMP_EMPTY, COMP_RECORD, COMP_SOLID, SELECT_BORDER, SELECT_LARGEST, SELECT_MIN_VOXELS, SIGHT_ALL, SKELETON_BORDER, SKELETON_BRANCH, SKELETON_BRANCH_BIT, SKELETON_CLOSED, SKELETON_NODE, SKELETON_SPUR, DIST_F32, DIST_SQ_I32, FILL_INTERIOR, FILL_SOLID, GEO_CHAMFER, GEO_FACES, GEO_NONE, GEO_SEEDS_BORDER, GEO_SEEDS_LIST, GEO_SEEDS_MASK, GEO_UNREACHED, ISO_GRID_DISTANCE, ISO_MESH_DISTANCE, ISO_SPACE_OBJECT, ISO_SPACE_VOXELS, MDIST_UNITS_F32, MDIST_VOXELS_F32, MEASURE_RECORD, MORPH_CLOSE, MORPH_DILATE, MORPH_ERODE, MORPH_OPEN, MODE_PARITY, MODE_REFERENCE, MODE_REFERENCE_SURFACE, MODE_SURFACE, PART_REGION, PART_THROAT, THIN_CURVE, THIN_KERNEL, Voxelizer, betti_numbers, intrusion_curve, mass_properties, obj_load, pore_network, sight_axes, sight_bit, skeleton_graph, thickness_voxels  # noqa: F401
