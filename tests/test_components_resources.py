"""The connected-component kernels (csrc/components.hip, with the numbering, `first` and edit kernels of csrc/dxv_label.h it instantiates for one
kind of root) as the compiler made them for gfx950, from its resource remarks (build.kernel_resources): none uses scratch memory or LDS (the scan
between them is csrc/scan.hip's: tests/test_scan_resources.py), and the shared kernels stay within the registers the skeleton's bounds give
their two-kind instances (tests/test_skeleton_resources.py).  The cross-compile needs no GPU."""
import os

# shared kernel -> (VGPR bound, waves per SIMD)
SHARED = {"k_label_roots": (8, 8), "k_label_number": (16, 8), "k_label_first": (16, 8), "k_label_edit": (24, 8)}


def test_components_kernels_use_no_scratch_memory(dxvlib):
    from dxrvoxelizer_amd import build
    if not os.path.exists(os.path.join(build.OBJDIR, "components.usage")):
        build.build(force=True)
    res = {k: v for k, v in build.kernel_resources("components").items() if "k_comp" in k or "k_label" in k}
    assert len(res) == 12, sorted(res)      # pack, init, merge, compress, stats_init, stats, table, keep; the shared roots, number, first, edit
    assert len([k for k in res if "k_label" in k]) == len(SHARED)
    for k, v in res.items():
        assert v["scratch"] == 0, k
        assert v["lds"] == 0, k
        for name, (vgprs, waves) in SHARED.items():
            if name in k:
                assert v["vgprs"] <= vgprs and v["occupancy"] >= waves, (k, v)
