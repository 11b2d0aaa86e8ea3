"""Every grid operator describes its scratch memory once, in a carve function (csrc/dxv_scratch.h and the X_carve beside each operator's
params).  tests/golden/operator_scratch.json is the record of what the two hand-written descriptions each operator had before -- X_scratch_bytes
and X_scratch_layout, or the pointer arithmetic inside its launcher -- gave: every total and every offset, for the sides 2 .. 1024 around every
word and tile boundary, both access forms, every morph op x form x radius, and the count pairs of the sized-later buffers.  The carves must
give the same bytes: the footprint and the alignment of every buffer are part of what the kernels were measured with."""
import json
import os
import subprocess

import pytest

import scratch_host

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROWS = json.load(open(os.path.join(ROOT, "tests", "golden", "operator_scratch.json")))
BASE = 1 << 40                                      # an address nobody touches: the carves only add to it
OPS = sorted({r["op"] for r in ROWS})


def rows_of(op):
    return [r for r in ROWS if r["op"] == op]


def test_the_table_covers_every_operator():
    assert OPS == sorted(["comp", "comp_select", "skel", "skel_prune", "oct", "iso", "thick", "part", "part_work", "access", "geo", "fill", "thin", "dist", "morph"])
    sides = {2, 4, 6, 8, 10, 14, 16, 18, 30, 32, 34, 62, 64, 66, 72, 126, 128, 130, 256, 510, 512, 1024}
    for op in ("comp", "skel", "oct", "iso", "thick", "part", "geo", "fill", "thin", "dist"):
        assert {r["args"][0] for r in rows_of(op)} == sides, op
    assert {tuple(r["args"]) for r in rows_of("access")} == {(n, i) for n in sides for i in (0, 1)}
    assert {tuple(r["args"]) for r in rows_of("morph")} == {(n, op, r2, form) for n in sides for op in range(4) for r2 in (1, 2, 9, 4096) for form in (1, 2)}
    pairs = {(0, 0), (1, 0), (0, 1), (1, 1), (255, 256), (257, 100000), (1 << 20, 1 << 24)}
    assert {tuple(r["args"]) for r in rows_of("part_work")} == pairs
    assert {tuple(r["args"]) for r in rows_of("skel_prune")} == pairs
    assert {r["args"][0] for r in rows_of("comp_select")} == {k for k, _ in pairs}


@pytest.mark.parametrize("op", OPS)
def test_totals_and_offsets_are_the_recorded_ones(op):
    for r in rows_of(op):
        want = dict(r["off"])
        if op == "oct":
            assert scratch_host.oct_levels(r["args"][0]) == want.pop("L")
        used, fits, off = scratch_host.carve(op, r["args"], BASE, r["total"])
        assert (used, off) == (r["total"], want), (op, r["args"])
        assert fits, (op, r["args"])


@pytest.mark.parametrize("op", OPS)
def test_the_sizing_run_and_the_layout_run_agree(op):
    for r in rows_of(op):
        sized, _, nothing = scratch_host.carve(op, r["args"])
        used, _, _ = scratch_host.carve(op, r["args"], BASE, r["total"])
        assert sized == used == r["total"], (op, r["args"])
        assert set(nothing.values()) == {-1}, (op, r["args"])         # over no base a carve hands out nothing


@pytest.mark.parametrize("op", OPS)
def test_one_byte_short_does_not_fit(op):
    for r in rows_of(op):
        used, fits, _ = scratch_host.carve(op, r["args"], BASE, r["total"] - 1)
        assert used == r["total"] and not fits, (op, r["args"])


def test_the_carves_are_clean_under_the_sanitizers(tmp_path):
    """a program of its own (its own main, nothing loaded into Python): every carve over an allocation of exactly its own size, both ends of
    every block written"""
    exe = tmp_path / "scratch_sanitize"
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wno-unknown-pragmas", "-o", str(exe),
                           os.path.join(ROOT, "tests", "cpp", "scratch_sanitize_main.cpp")])
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout[-1000:], r.stderr[-3000:])
    assert sorted(l.split(":")[0] for l in r.stdout.splitlines()) == OPS
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr
