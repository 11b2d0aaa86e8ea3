"""The thinning kernels (csrc/thin.hip) as the compiler made them for gfx950, from its resource remarks (build.kernel_resources): neither uses
scratch memory or LDS, and their registers stay within the bounds DESIGN §4.12 states (read off the build: 18 VGPRs for the border, 64 for a
sub-iteration, each bound the next multiple of eight; both at eight waves per SIMD).  The cross-compile needs no GPU."""
import os

VGPR_BOUND = {"k_thin_border": 24, "k_thin_sub": 64}


def test_thin_kernels_use_no_scratch_memory_and_no_lds(dxvlib):
    from dxrvoxelizer_amd import build
    if not os.path.exists(os.path.join(build.OBJDIR, "thin.usage")):
        build.build(force=True)
    res = {k: v for k, v in build.kernel_resources("thin").items() if "k_thin" in k}
    assert len(res) == 2, sorted(res)                                  # border, sub
    for k, v in res.items():
        bound = next(b for name, b in VGPR_BOUND.items() if name in k)
        assert v["scratch"] == 0, k
        assert v["lds"] == 0, k
        assert v["vgprs"] <= bound, (k, v["vgprs"])
        assert v["occupancy"] == 8, (k, v["occupancy"])
