"""The partition kernels (csrc/partition.hip) as the compiler made them for gfx950, from its resource remarks (build.kernel_resources): none uses
scratch memory, their LDS is the few words of a block's scan, and their registers stay within the bounds DESIGN §4.16 states (read off the build;
each bound the next multiple of eight).  The scan of the blocks' sums is csrc/scan.hip's: tests/test_scan_resources.py.  The cross-compile needs
no GPU."""
import os

# kernel -> (VGPR bound, waves per SIMD, LDS bytes at the most)
BOUND = {"k_part_keys": (16, 8, 0), "k_part_mip": (16, 8, 0), "k_part_searchILb0E": (128, 4, 0), "k_part_searchILb1E": (152, 3, 0), "k_part_walk": (8, 8, 0),
         "k_part_countILb0E": (16, 8, 16), "k_part_countILb1E": (24, 8, 16), "k_part_number": (16, 8, 16), "k_part_labels": (8, 8, 0),
         "k_part_stats_init": (16, 8, 0), "k_part_statsE": (16, 8, 0), "k_part_table": (16, 8, 0), "k_part_emit_faces": (32, 8, 16), "k_part_count_heads": (16, 8, 16),
         "k_part_emit_pairs": (16, 8, 16), "k_part_face_atomics": (24, 8, 0), "k_part_throatsE": (16, 8, 0)}
ROW = {"k_part_searchILb0E": "k_part_search<false>", "k_part_searchILb1E": "k_part_search<true>", "k_part_countILb0E": "k_part_count<false>", "k_part_countILb1E": "k_part_count<true>",
       "k_part_statsE": "k_part_stats", "k_part_throatsE": "k_part_throats"}


def test_partition_kernels_use_no_scratch_memory_and_stay_within_their_registers(dxvlib):
    from dxrvoxelizer_amd import build
    if not os.path.exists(os.path.join(build.OBJDIR, "partition.usage")):
        build.build(force=True)
    res = {k: v for k, v in build.kernel_resources("partition").items() if "k_part" in k}
    assert len(res) == len(BOUND), sorted(res)
    for k, v in res.items():
        hits = [(n, b) for n, b in BOUND.items() if n in k]
        assert len(hits) == 1, (k, hits)
        name, (vgprs, waves, lds) = hits[0]
        assert v["scratch"] == 0, k
        assert v["lds"] <= lds, (k, v["lds"])
        assert v["vgprs"] <= vgprs, (k, v["vgprs"])
        assert v["occupancy"] >= waves, (k, v["occupancy"])


def test_the_bounds_are_the_numbers_in_the_design_document():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with open(os.path.join(root, "DESIGN.md")) as fh:
        design = fh.read()
    section = design[design.index("### 4.16"):]
    for name, (vgprs, waves, _) in BOUND.items():
        shown = ROW.get(name, name)
        row = next(line for line in section.splitlines() if line.startswith(f"| `{shown}`"))
        cells = [c.strip() for c in row.strip("|").split("|")]
        assert int(cells[2]) <= vgprs and -(-int(cells[2]) // 8) * 8 == vgprs and int(cells[3]) == waves, row
