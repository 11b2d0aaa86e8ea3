"""The octree kernels (csrc/octree.hip) as the compiler made them for gfx950, from its resource remarks (build.kernel_resources): none uses
scratch memory or LDS (the scan between them is csrc/scan.hip's: tests/test_scan_resources.py).  The cross-compile needs no GPU."""
import os


def test_octree_kernels_use_no_scratch_memory(dxvlib):
    from dxrvoxelizer_amd import build
    if not os.path.exists(os.path.join(build.OBJDIR, "octree.usage")):
        build.build(force=True)
    res = {k: v for k, v in build.kernel_resources("octree").items() if "k_oct" in k}
    assert len(res) == 6, sorted(res)                                  # reduce, level, flags, level_first, emit, expand
    for k, v in res.items():
        assert v["scratch"] == 0, k
        assert v["lds"] == 0, k
