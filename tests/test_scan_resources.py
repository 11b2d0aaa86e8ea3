"""The scan kernels (csrc/scan.hip) as the compiler made them for gfx950, from its resource remarks (build.kernel_resources): three kernels for one
and for two interleaved counts per word, none uses scratch memory, their LDS is exactly the waves' sums of csrc/dxv_scan.h -- 8 bytes per count
and wave --, and their registers stay within the bounds DESIGN §4.17 states (read off the build; each bound the next multiple of eight).  The
one-workgroup kernel for two counts stands where k_thick_scan and k_part_scan stood, and within what was recorded for them: 78 VGPRs, six waves
per SIMD, 256 bytes of LDS.  The cross-compile needs no GPU."""
import os

# kernel (as mangled: ILj<C>E) -> (VGPR bound, waves per SIMD, waves of a workgroup, counts per word)
BOUND = {"k_scan_block_sumsILj1E": (16, 8, 4, 1), "k_scan_sumsILj1E": (48, 8, 16, 1), "k_scan_addILj1E": (24, 8, 4, 1),
         "k_scan_block_sumsILj2E": (24, 8, 4, 2), "k_scan_sumsILj2E": (80, 6, 16, 2), "k_scan_addILj2E": (48, 8, 4, 2)}


def shown(name):
    return name.replace("ILj1E", "<1>").replace("ILj2E", "<2>")


def test_scan_kernels_use_no_scratch_memory_and_stay_within_their_registers(dxvlib):
    from dxrvoxelizer_amd import build
    if not os.path.exists(os.path.join(build.OBJDIR, "scan.usage")):
        build.build(force=True)
    res = {k: v for k, v in build.kernel_resources("scan").items() if "k_scan" in k}
    assert len(res) == len(BOUND), sorted(res)
    for k, v in res.items():
        hits = [(n, b) for n, b in BOUND.items() if n in k]
        assert len(hits) == 1, (k, hits)
        name, (vgprs, waves, group, lanes) = hits[0]
        assert v["scratch"] == 0, k
        assert v["lds"] == group * 8 * lanes, (k, v["lds"])
        assert v["vgprs"] <= vgprs, (k, v["vgprs"])
        assert v["occupancy"] >= waves, (k, v["occupancy"])


def test_the_bounds_are_the_numbers_in_the_design_document():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with open(os.path.join(root, "DESIGN.md")) as fh:
        design = fh.read()
    section = design[design.index("### 4.17"):]
    for name, (vgprs, waves, group, lanes) in BOUND.items():
        row = next(line for line in section.splitlines() if line.startswith(f"| `{shown(name)}`"))
        cells = [c.strip() for c in row.strip("|").split("|")]
        assert int(cells[2]) <= vgprs and -(-int(cells[2]) // 8) * 8 == vgprs and int(cells[3]) == waves and int(cells[4]) == group * 8 * lanes, row
