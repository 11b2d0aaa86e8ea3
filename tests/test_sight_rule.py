"""The line-of-sight rule on the CPU: the product's routines (csrc/dxv_sight.h through tests/sight_host.py, run word by word as the device
runs them, the grouped carry included) against the two restatements of tests/sight_restated.py -- (a) the literal line walk, (b) the plane
recurrence -- and the rule's own properties: a subset's map is the full map masked, mirroring the grid permutes the bits as the numbering
says, the edit leaves nothing hidden, the scratch carve sizes and lays out alike."""
import os
import subprocess

import numpy as np
import pytest

import grid_sides as gs
import sight_host as sh
import sight_restated as sr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KINDS = (sr.SOLID, sr.EMPTY)
PAIRS = [sr.axis_bits(a) for a in range(13)]


def small_grid(N, seed, density):
    rng = np.random.default_rng(seed)
    return (rng.random((N, N, N)) < density).astype(np.uint8) * rng.integers(1, 256, (N, N, N), dtype=np.uint8)


def same(got, want_map, g, of, directions, key):
    field, tally = got
    assert field.dtype == np.uint32 and field.tobytes() == want_map.tobytes(), (key, int(np.count_nonzero(field != want_map)))
    assert sr.same_tally(tally, sr.tally(g, of, want_map, directions)), key


def test_the_numbering():
    lib = sh.library()
    assert lib.sc_all() == sr.ALL == sum(1 << b for b in sr.BITS) and lib.sc_max_n() == 1024
    seen = set()
    for dz in (-1, 0, 1):
        for dy in (-1, 0, 1):
            for dx in (-1, 0, 1):
                b = lib.sc_bit(dx, dy, dz)
                assert b == sr.bit(dx, dy, dz) and sr.direction(b) == (dx, dy, dz) and lib.sc_bit(-dx, -dy, -dz) == 26 - b
                seen.add(b)
    assert seen == set(range(27)) and sr.bit(0, 0, 0) == 13
    assert sorted(PAIRS) == sorted({(1 << b) | (1 << (26 - b)) for b in sr.BITS})
    assert [lib.sc_group(W, 0) for W in (1, 2, 3, 4, 5, 8, 9, 16)] == [1, 2, 4, 4, 8, 8, 16, 16] and lib.sc_group(2, 16) == 16 and lib.sc_group(5, 2) == 8


@pytest.mark.parametrize("N", [2, 4, 6, 8])
def test_the_host_library_is_the_line_walk_and_the_recurrence(N):
    for seed, density in ((N, 0.25), (N + 1, 0.6), (N + 2, 0.05)):
        g = small_grid(N, seed, density)
        for of in KINDS:
            a, b = sr.walk(g, of, sr.ALL), sr.sight(g, of, sr.ALL)
            assert a.tobytes() == b.tobytes(), (N, seed, of)
            same(sh.sight(g, of, sr.ALL), a, g, of, sr.ALL, (N, seed, of))
            for directions in [1 << k for k in sr.BITS] + PAIRS:
                assert sr.walk(g, of, directions).tobytes() == (a & np.uint32(directions)).tobytes()
                same(sh.sight(g, of, directions), a & np.uint32(directions), g, of, directions, (N, seed, of, directions))


@pytest.mark.parametrize("N", gs.SWEEP + gs.WIDE)
def test_every_side_of_the_sweep(N):
    """host library == (b) on every grid of the side, both kinds; below 30 every single direction and pair too; at four sides every group
    width on every grid but the one of members only (at 130: rows of three words in groups of 4, 8 and 16, on random content and on "ends")"""
    for name, g in gs.grids(N, None if N <= 72 else gs.WIDE_GRIDS):
        for of in KINDS:
            want = sr.sight(g, of, sr.ALL)
            same(sh.sight(g, of, sr.ALL), want, g, of, sr.ALL, (N, name, of))
            if N < 30 and name in ("random 0.3", "ends"):
                for directions in [1 << k for k in sr.BITS] + PAIRS:
                    same(sh.sight(g, of, directions), want & np.uint32(directions), g, of, directions, (N, name, of, directions))
            if N in (2, 20, 66, 130) and name != "all 0xFF":
                for group in (1, 2, 4, 8, 16):
                    got = sh.sight(g, of, sr.ALL, group)
                    assert got[0].tobytes() == want.tobytes(), (N, name, of, group)


@pytest.mark.parametrize("N", [6, 16, 66])
def test_mirroring_the_grid_permutes_the_bits(N):
    g = gs.random_grid(N, 0.3)
    for of in KINDS:
        base = sh.sight(g, of, sr.ALL)[0]
        for axis, flip in (("x", 2), ("y", 1), ("z", 0)):
            got = sh.sight(np.ascontiguousarray(np.flip(g, flip)), of, sr.ALL)[0]
            assert np.flip(got, flip).tobytes() == sr.mirrored_bits(base, axis).tobytes(), (N, of, axis)


def test_the_conditions_of_the_device_tests_hold():
    """what tests/test_gpu_sight.py asserts of its inputs, here from the restatement at two sides"""
    for N in (16, 66):
        t = sr.tally(gs.random_grid(N, 0.3), sr.EMPTY, sr.sight(gs.random_grid(N, 0.3), sr.EMPTY), sr.ALL)
        assert np.count_nonzero(t["count"]) >= 10 and len({int(t["seen"][b]) for b in sr.BITS}) >= 2, (N, t)
    box = gs.hollow_box(16, 2, 6)                                        # (off the diagonals of the corner voxel (z, y, x) = (0, 15, 15))
    t = sr.tally(box, sr.EMPTY, sr.sight(box, sr.EMPTY), sr.ALL)
    assert t["count"][0] == 3 ** 3 and t["count"][26] > 0


@pytest.mark.parametrize("N", [6, 16, 34])
def test_after_the_edit_nothing_is_hidden(N):
    for name, g in list(gs.grids(N, ("random 0.3", "hollow box"))) + [("t slot", sr.t_slot(16))]:
        for of in KINDS:
            for directions in (sr.ALL, PAIRS[8], 1 << sr.bit(0, 0, -1), PAIRS[0] | PAIRS[2]):
                field = sh.sight(g, of, sr.ALL)[0]
                edited = sh.sight_fill(g, of, directions, field)
                assert edited.tobytes() == sr.sight_fill(g, of, field, directions).tobytes(), (N, name, of, directions)
                again, tally = sh.sight(edited, of, directions)
                assert tally["count"][0] == 0, (N, name, of, directions)
                # a member that was seen stays one, with the same bits
                kept = (field & np.uint32(directions)) != 0
                assert ((again & np.uint32(directions))[kept] == (field & np.uint32(directions))[kept]).all()


def test_the_builders():
    slot = sr.t_slot(16)
    field, tally = sh.sight(slot, sr.EMPTY, sr.ALL)
    assert tally["neither"][0] == 0 and tally["neither"][2] == tally["members"] > 0 and tally["neither"][8] > 0
    assert sr.direction(14 + 0) == (1, 0, 0) and sr.direction(14 + 2) == (0, 1, 0) and sr.direction(14 + 8) == (0, 0, 1)
    assert int(np.argmin(tally["neither"])) == 0 and np.count_nonzero(tally["neither"] == 0) == 1
    assert int(np.argmax(tally["neither"])) == 2 and np.count_nonzero(tally["neither"] == tally["members"]) == 1
    plate = sr.plate_with_pinhole(16, (5, 9))
    down = 1 << sr.bit(0, 0, -1)                                         # rays travelling down z: from above
    field = sh.sight(plate, sr.EMPTY, down)[0]
    below = field[:8] != 0
    assert below[:, 5, 9].all() and below.sum() == 8 and (field[9:] == down).all()


def test_refusals():
    lib = sh.library()
    assert lib.sc_valid(2, 0, 1) == 1 and lib.sc_valid(1024, 1, sr.ALL) == 1
    for bad in ((0, 0, 1), (3, 0, 1), (1026, 0, 1), (16, 2, 1), (16, -1, 1), (16, 0, 0), (16, 0, 1 << 13), (16, 0, 1 << 27), (16, 0, 0xFFFFFFFF)):
        assert lib.sc_valid(*bad) == 0, bad


@pytest.mark.parametrize("N", [2, 6, 64, 66, 130, 1024])
def test_the_scratch_is_sized_and_laid_out_alike(N):
    for directions in (1, PAIRS[3], sr.ALL):
        total, fits, _ = sh.carve(N, directions)
        words = N * N * ((N + 63) // 64)
        assert total >= 68 * 8 + 8 * words * (1 + bin(directions).count("1")) and total % 256 == 0 and not fits
        base = 1 << 40
        used, fits, blocks = sh.carve(N, directions, base, total)
        assert used == total and fits and blocks[0] == base and blocks[0] < blocks[1] < blocks[2] and all(b % 256 == 0 for b in blocks)
        assert blocks[1] - blocks[0] >= 68 * 8 and blocks[2] - blocks[1] >= 8 * words and base + total - blocks[2] >= 8 * words * bin(directions).count("1")
        used, fits, _ = sh.carve(N, directions, base, total - 1)
        assert used == total and not fits


def test_the_host_routines_are_clean_under_the_sanitizers(tmp_path):
    """a program of its own (its own main, nothing loaded into Python): sides 2, 62, 64, 66 and 130, every block of the scratch written at
    both ends over an allocation of exactly its size"""
    exe = tmp_path / "sight_sanitize"
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wno-unknown-pragmas", "-o", str(exe),
                           os.path.join(ROOT, "tests", "cpp", "sight_sanitize_main.cpp")])
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout[-1000:], r.stderr[-3000:])
    assert len(r.stdout.splitlines()) == 5 * 2 * 2
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr
