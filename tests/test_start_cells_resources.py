"""Registers and static instructions of the brick kernels around the start cells (dxv_dirmap.h: dm_ray_start<2>), from the compiler's own
remarks (dxrvoxelizer_amd/build.py) and its gfx950 assembly (tools/isa_counts.py); no GPU.

The kernels that read the table read ONE cell per ray: they must issue exactly as many vector load instructions as their _plain twins (with
the 4-byte word beside the cell they issued one more), hold no scratch, and keep their waves -- 64 VGPRs for k_voxelize_listed<false> (the
eighth wave), 68 for k_voxelize_queue<false>, 72 for both texel variants.  The _plain kernels are not this change's business: their
registers are what they were, and no class of their instructions has grown.  (Their numbers below are those of the commit before the start
cells; k_voxelize_listed_plain<false> has three scalar instructions fewer since -- the parameter block grew by one pointer and the
compiler groups its scalar loads, and the waits behind them, differently.)"""
import os
import sys

import pytest

from dxrvoxelizer_amd import build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

LISTED = "NS_14VoxelizeParamsENS_9QueueLensENS_10ClearShareE"
QUEUE = "NS_14VoxelizeParamsE"
TABLE_CEILINGS = {"k_voxelize_listedILb0EEEv" + LISTED: (64, 8), "k_voxelize_listedILb1EEEv" + LISTED: (72, 7),
                  "k_voxelize_queueILb0EEEv" + QUEUE: (68, 7), "k_voxelize_queueILb1EEEv" + QUEUE: (72, 7)}
# the _plain kernels before the start cells: VGPRs, SGPRs; vector ALU, scalar, vector loads, vector stores + atomics, LDS, divisions
PLAIN_BEFORE = {"k_voxelize_listed_plainILb0EEEv" + LISTED: (64, 79, 1508, 1282, 25, 74, 39, 7),
                "k_voxelize_listed_plainILb1EEEv" + LISTED: (72, 79, 1439, 1288, 21, 75, 44, 6),
                "k_voxelize_queue_plainILb0EEEv" + QUEUE: (68, 90, 931, 685, 23, 6, 7, 7),
                "k_voxelize_queue_plainILb1EEEv" + QUEUE: (72, 88, 873, 690, 19, 7, 7, 6)}


def one(table, fragment):
    got = [v for k, v in table.items() if fragment in k]
    assert len(got) == 1, (fragment, sorted(table))
    return got[0]


@pytest.fixture(scope="module")
def usage(dxvlib):
    if not os.path.exists(os.path.join(build.OBJDIR, "voxelize_lists.usage")):
        build.build(force=True)
    return build.kernel_resources("voxelize_lists")


@pytest.fixture(scope="module")
def counts():
    from tools import isa_counts
    return isa_counts.counts(isa_counts.assembly("voxelize_lists.hip"), ["k_voxelize_listed", "k_voxelize_queue"])


def test_table_kernels_keep_their_waves(usage):
    for fragment, (vgprs, waves) in TABLE_CEILINGS.items():
        r = one(usage, fragment)
        print(fragment, r)
        assert r["scratch"] == 0 and r["vgprs"] <= vgprs and r["occupancy"] >= waves, (fragment, r)


def test_plain_kernels_registers_are_what_they_were(usage):
    for fragment, before in PLAIN_BEFORE.items():
        r = one(usage, fragment)
        print(fragment, r)
        assert r["scratch"] == 0 and r["vgprs"] == before[0] and r["sgprs"] == before[1], (fragment, r)


def test_one_cell_load_and_plain_instruction_counts(counts):
    for fragment, before in PLAIN_BEFORE.items():
        plain, table = one(counts, fragment), one(counts, fragment.replace("_plain", ""))
        print(fragment, plain, table)
        # the table kernels: the cell is their only load in front of the scan, as it is the plain kernels'
        assert table["vector_loads"] == plain["vector_loads"], (fragment, table, plain)
        now = tuple(plain.get(k, 0) for k in ("valu", "salu", "vector_loads", "vector_stores", "lds", "divisions_f32"))
        assert now[2] == before[4], (fragment, now)
        assert all(a <= b for a, b in zip(now, before[2:])), (fragment, now, before[2:])
