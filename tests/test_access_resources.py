"""The access kernels (csrc/access.hip) as the compiler made them for gfx950, from its resource remarks (build.kernel_resources): none uses
scratch memory, the round kernel's LDS is its tile with the halo (10^3 words) and the word of its flags, the tally's is its four partial
tallies, and their registers stay within the bounds DESIGN §4.18 states (read off the build; each bound the next multiple of eight).  The
cross-compile needs no GPU."""
import os

# kernel -> (VGPR bound, waves per SIMD, LDS bytes at the most)
BOUND = {"k_acc_init": (16, 8, 0), "k_acc_seed_list": (16, 8, 0), "k_acc_roundILi6E": (96, 5, 4004), "k_acc_roundILi26E": (112, 4, 4004), "k_acc_tally": (40, 8, 128),
         "k_acc_radius": (16, 8, 0)}
ROW = {"k_acc_roundILi6E": "k_acc_round<6>", "k_acc_roundILi26E": "k_acc_round<26>"}


def test_access_kernels_use_no_scratch_memory_and_stay_within_their_registers(dxvlib):
    from dxrvoxelizer_amd import build
    if not os.path.exists(os.path.join(build.OBJDIR, "access.usage")):
        build.build(force=True)
    res = {k: v for k, v in build.kernel_resources("access").items() if "k_acc" in k}
    assert len(res) == len(BOUND), sorted(res)
    for k, v in res.items():
        name, (vgprs, waves, lds) = next((n, b) for n, b in BOUND.items() if n in k)
        assert v["scratch"] == 0, k
        assert v["lds"] <= lds, (k, v["lds"])
        assert v["vgprs"] <= vgprs, (k, v["vgprs"])
        assert v["occupancy"] >= waves, (k, v["occupancy"])
    assert 4004 == 4 * 10 ** 3 + 4                                      # the tile plus its flags


def test_the_bounds_are_the_numbers_in_the_design_document():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with open(os.path.join(root, "DESIGN.md")) as fh:
        design = fh.read()
    section = design[design.index("### 4.18"):]
    for name, (vgprs, waves, _) in BOUND.items():
        row = next(line for line in section.splitlines() if line.startswith(f"| `{ROW.get(name, name)}`"))
        cells = [c.strip() for c in row.strip("|").split("|")]
        assert int(cells[2]) <= vgprs and -(-int(cells[2]) // 8) * 8 == vgprs and int(cells[3]) == waves, row
