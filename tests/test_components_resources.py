"""The connected-component kernels (csrc/components.hip) as the compiler made them for gfx950, from its resource remarks
(build.kernel_resources): none uses scratch memory or LDS (the scan between them is csrc/scan.hip's: tests/test_scan_resources.py).  The
cross-compile needs no GPU."""
import os


def test_components_kernels_use_no_scratch_memory(dxvlib):
    from dxrvoxelizer_amd import build
    if not os.path.exists(os.path.join(build.OBJDIR, "components.usage")):
        build.build(force=True)
    res = {k: v for k, v in build.kernel_resources("components").items() if "k_comp" in k}
    assert len(res) == 12, sorted(res)      # pack, init, merge, compress, roots, number, stats_init, first, stats, table, keep, edit
    for k, v in res.items():
        assert v["scratch"] == 0, k
        assert v["lds"] == 0, k
