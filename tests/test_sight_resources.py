"""The line-of-sight kernels (csrc/sight.hip) as the compiler made them for gfx950, from its resource remarks (build.kernel_resources): none
uses scratch memory, the tally alone uses LDS -- its four waves' 68 partial sums --, and their registers stay within the bounds DESIGN §4.20
states (read off the build; each bound the next multiple of eight).  The cross-compile needs no GPU."""
import os

# kernel -> (VGPR bound, waves per SIMD, LDS bytes at the most)
BOUND = {"k_sight_pack": (24, 8, 0), "k_sight_sweep": (40, 8, 0), "k_sight_map": (40, 8, 0), "k_sight_tally": (168, 3, 4 * 68 * 4), "k_sight_fill": (8, 8, 0)}


def test_sight_kernels_use_no_scratch_memory_and_stay_within_their_registers(dxvlib):
    from dxrvoxelizer_amd import build
    if not os.path.exists(os.path.join(build.OBJDIR, "sight.usage")):
        build.build(force=True)
    res = {k: v for k, v in build.kernel_resources("sight").items() if "k_sight" in k}
    assert len(res) == len(BOUND), sorted(res)
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
    section = design[design.index("### 4.20"):]
    for name, (vgprs, waves, _) in BOUND.items():
        row = next(line for line in section.splitlines() if line.startswith(f"| `{name}`"))
        cells = [c.strip() for c in row.strip("|").split("|")]
        assert int(cells[2]) <= vgprs and -(-int(cells[2]) // 8) * 8 == vgprs and int(cells[3]) == waves, row
