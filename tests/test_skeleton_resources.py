"""The skeleton kernels (csrc/skeleton.hip, with the numbering, `first` and edit kernels of csrc/dxv_label.h it instantiates for two kinds of
root) as the compiler made them for gfx950, from its resource remarks (build.kernel_resources): none uses
scratch memory, none uses LDS -- the classify kernel least of all: its 27 words and its counter are registers --, and their registers stay within
the bounds DESIGN §4.19 states (read off the build; each bound the next multiple of eight).  The cross-compile needs no GPU."""
import os

# kernel -> (VGPR bound, waves per SIMD)
BOUND = {"k_skel_classify": (64, 8), "k_skel_init": (24, 8), "k_label_roots": (8, 8), "k_label_number": (16, 8), "k_skel_stats_init": (16, 8), "k_label_first": (16, 8),
         "k_skel_statsE": (72, 7), "k_skel_nodes": (16, 8), "k_skel_branches": (16, 8), "k_skel_prune_mark": (16, 8), "k_label_edit": (24, 8)}
ROW = {"k_skel_statsE": "k_skel_stats", "k_label_roots": "k_label_roots<2>", "k_label_number": "k_label_number<2>", "k_label_first": "k_label_first<2>",
       "k_label_edit": "k_label_edit<SkelGoes>"}


def test_skeleton_kernels_use_no_scratch_memory_no_lds_and_stay_within_their_registers(dxvlib):
    from dxrvoxelizer_amd import build
    if not os.path.exists(os.path.join(build.OBJDIR, "skeleton.usage")):
        build.build(force=True)
    res = {k: v for k, v in build.kernel_resources("skeleton").items() if "k_skel" in k or "k_label" in k}
    assert len(res) == len(BOUND), sorted(res)
    for k, v in res.items():
        name, (vgprs, waves) = next((n, b) for n, b in BOUND.items() if n in k)
        assert v["scratch"] == 0, k
        assert v["lds"] == 0, (k, v["lds"])
        assert v["vgprs"] <= vgprs, (k, v["vgprs"])
        assert v["occupancy"] >= waves, (k, v["occupancy"])


def test_the_bounds_are_the_numbers_in_the_design_document():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with open(os.path.join(root, "DESIGN.md")) as fh:
        design = fh.read()
    section = design[design.index("### 4.19"):]
    for name, (vgprs, waves) in BOUND.items():
        row = next(line for line in section.splitlines() if line.startswith(f"| `{ROW.get(name, name)}`"))
        cells = [c.strip() for c in row.strip("|").split("|")]
        assert int(cells[2]) <= vgprs and -(-int(cells[2]) // 8) * 8 == vgprs and int(cells[3]) == waves, row
