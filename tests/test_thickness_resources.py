"""The thickness kernels (csrc/thickness.hip) as the compiler made them for gfx950, from its resource remarks (build.kernel_resources): none uses
scratch memory, only the scans inside a block (16 bytes) and the histogram (16,388 bytes: cap + 1 = 4097 bins of 32 bits) use LDS, and their
registers stay within the bounds DESIGN §4.14 states (read off the build: 7, 16, 32, 11, 18 and 10 VGPRs; each bound the next multiple of eight;
eight waves per SIMD).  The scan of the blocks' sums is csrc/scan.hip's: tests/test_scan_resources.py.  The cross-compile needs no GPU."""
import os

# kernel -> (VGPR bound, waves per SIMD, LDS bytes at the most)
BOUND = {"k_thick_members": (8, 8, 0), "k_thick_top": (16, 8, 0), "k_thick_select": (32, 8, 16), "k_thick_emit": (16, 8, 16),
         "k_thick_paint": (24, 8, 0), "k_thick_histogram": (16, 8, 16388)}


def test_thickness_kernels_use_no_scratch_memory_and_stay_within_their_registers(dxvlib):
    from dxrvoxelizer_amd import build
    if not os.path.exists(os.path.join(build.OBJDIR, "thickness.usage")):
        build.build(force=True)
    res = {k: v for k, v in build.kernel_resources("thickness").items() if "k_thick" in k}
    assert len(res) == len(BOUND) + 1, sorted(res)                     # (the paint twice: without and with its counters)
    for k, v in res.items():
        name, (vgprs, waves, lds) = next((n, b) for n, b in BOUND.items() if n in k)
        assert v["scratch"] == 0, k
        assert v["lds"] <= lds, (k, v["lds"])
        assert v["vgprs"] <= vgprs, (k, v["vgprs"])
        assert v["occupancy"] >= waves, (k, v["occupancy"])


def test_the_bounds_are_the_numbers_in_the_design_document():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with open(os.path.join(root, "DESIGN.md")) as fh:
        design = fh.read()
    section = design[design.index("### 4.14"):]
    for name, (vgprs, waves, _) in BOUND.items():
        row = next(line for line in section.splitlines() if line.startswith(f"| `{name}`"))
        cells = [c.strip() for c in row.strip("|").split("|")]
        assert int(cells[2]) <= vgprs and -(-int(cells[2]) // 8) * 8 == vgprs and int(cells[3]) == waves, row
