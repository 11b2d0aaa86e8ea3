"""The morphology kernels (csrc/morph.hip) as the compiler made them for gfx950, from its resource remarks (build.kernel_resources): none uses
scratch memory or LDS, and their registers stay within the bounds DESIGN §4.11 states (read off the build: 20, 20, 13, 12 and 14 VGPRs for
pack, spread, ball, write and threshold, each bound the next multiple of eight; every kernel at eight waves per SIMD).  The cross-compile needs no GPU."""
import os

VGPR_BOUND = {"k_morph_pack": 24, "k_morph_spread": 24, "k_morph_ball": 16, "k_morph_write": 16, "k_morph_threshold": 16}


def test_morph_kernels_use_no_scratch_memory_and_no_lds(dxvlib):
    from dxrvoxelizer_amd import build
    if not os.path.exists(os.path.join(build.OBJDIR, "morph.usage")):
        build.build(force=True)
    res = {k: v for k, v in build.kernel_resources("morph").items() if "k_morph" in k}
    assert len(res) == 5, sorted(res)                                  # pack, spread, ball, write, threshold
    for k, v in res.items():
        bound = next(b for name, b in VGPR_BOUND.items() if name in k)
        assert v["scratch"] == 0, k
        assert v["lds"] == 0, k
        assert v["vgprs"] <= bound, (k, v["vgprs"])
        assert v["occupancy"] == 8, (k, v["occupancy"])
