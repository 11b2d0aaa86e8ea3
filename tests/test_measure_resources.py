"""The measure kernels (csrc/measure.hip) as the compiler made them for gfx950, from its resource remarks (build.kernel_resources): none uses
scratch memory or LDS, and their registers stay within the bounds DESIGN §4.13 states (read off the build: 108 VGPRs for k_measure at
connectivity 6, 123 at 26 -- the 26 words of owned cells of a mask word are live across its runs --, 72 for the total; each bound the next
multiple of eight; four, four and seven waves per SIMD).  The cross-compile needs no GPU."""
import os

VGPR_BOUND = {"k_measureILj6E": (112, 4), "k_measureILj26E": (128, 4), "k_measure_total": (72, 7)}


def test_measure_kernels_use_no_scratch_memory_and_no_lds(dxvlib):
    from dxrvoxelizer_amd import build
    if not os.path.exists(os.path.join(build.OBJDIR, "measure.usage")):
        build.build(force=True)
    res = {k: v for k, v in build.kernel_resources("measure").items() if "k_measure" in k}
    assert len(res) == 3, sorted(res)                                  # k_measure<6>, k_measure<26>, total
    for k, v in res.items():
        bound, waves = next(b for name, b in VGPR_BOUND.items() if name in k)
        assert v["scratch"] == 0, k
        assert v["lds"] == 0, k
        assert v["vgprs"] <= bound, (k, v["vgprs"])
        assert v["occupancy"] >= waves, (k, v["occupancy"])
