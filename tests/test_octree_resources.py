"""The octree kernels (csrc/octree.hip) as the compiler made them for gfx950, from its resource remarks (build.kernel_resources): none uses
scratch memory.  The cross-compile needs no GPU."""
import os


def test_octree_kernels_use_no_scratch_memory(dxvlib):
    from dxrvoxelizer_amd import build
    if not os.path.exists(os.path.join(build.OBJDIR, "octree.usage")):
        build.build(force=True)
    res = {k: v for k, v in build.kernel_resources("octree").items() if "k_oct" in k}
    assert len(res) == 9, sorted(res)                                  # reduce, level, flags, the scan's three, level_first, emit, expand
    for k, v in res.items():
        assert v["scratch"] == 0, k
        assert v["lds"] <= 128, k                                      # the scan's wave sums; the others use none
