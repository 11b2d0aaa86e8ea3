"""Topology-preserving thinning (include/dxv.h: dxv_thin) on the CPU: what the numpy restatement (tests/thin_restated.py) must keep
-- a subset, idempotent, pieces, cavities and Euler characteristic unchanged, the composition law of max_iterations, a voxel for a blob and a
ring for a torus --, the product's word routines (csrc/dxv_thin.h compiled for the CPU: tests/thin_host.py) against it in grid, iterations and
removed, that the subfield order matters, and what the header declares."""
import os
import re
import subprocess

import numpy as np
import pytest

import grid_sides as gs
import thin_host
import thin_restated as tr
import thin_shapes as ts
from conftest import ROOT

SIDES = (2, 6, 12, 16, 24)


# ---- the restatement ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", SIDES)
def test_restatement_keeps_topology_and_composes(N):
    for what, g in ts.shapes(N):
        solid = g != 0
        before = tr.topology(g)
        for kind in tr.KINDS:
            out, iterations, removed, converged = tr.thin(g, kind)
            assert out.dtype == np.uint8 and out.max(initial=0) <= 1 and converged and iterations >= 1, (N, what, kind)
            assert not ((out != 0) & ~solid).any(), (N, what, kind)     # a subset of the input
            assert removed == tr.counts(g, out), (N, what, kind)
            assert tr.topology(out) == before, (N, what, kind)
            again = tr.thin(out, kind)
            assert np.array_equal(again[0], out) and again[1:] == (1, 0, True), (N, what, kind)
            for a, b in ((1, 1), (2, 1), (1, 3)):
                whole = tr.thin(g, kind, a + b)
                first = tr.thin(g, kind, a)
                assert np.array_equal(tr.thin(first[0], kind, b)[0], whole[0]), (N, what, kind, a, b)
                assert whole[1] <= a + b and (whole[3] or whole[1] == a + b), (N, what, kind, a, b)
                assert tr.topology(first[0]) == before, (N, what, kind, a)


@pytest.mark.parametrize("N", SIDES)
def test_kernel_of_a_blob_is_one_voxel_and_of_a_torus_a_ring(N):
    for what, g in (("full", ts.full(N)), ("ball", ts.ball(N))):
        assert g.any(), (N, what)
        out = tr.thin(g, tr.KERNEL)[0]
        assert int(out.sum()) == 1, (N, what)
    if N >= 12:
        torus = ts.torus(N)
        assert tr.topology(torus) == (1, 1, 0)                          # one piece, no cavity, one tunnel
        ring = tr.thin(torus, tr.KERNEL)[0]
        assert ring.any() and set(tr.neighbours26(ring)[ring != 0].tolist()) == {2}, N
        assert tr.topology(ring) == (1, 1, 0)
    shell = tr.thin(ts.shell(N), tr.KERNEL)[0]
    assert tr.topology(shell) == tr.topology(ts.shell(N))
    if N >= 12:
        assert tr.topology(shell)[1] == 2 and tr.topology(shell)[2] == 2      # a closed sheet round a cavity stays one


@pytest.mark.parametrize("N", SIDES)
def test_curve_leaves_the_one_voxel_cross_as_it_is(N):
    g = ts.cross(N)
    out, iterations, removed, converged = tr.thin(g, tr.CURVE)
    if N == 2:                                                          # arms of one voxel: the three arm voxels touch each other along edges, a clump and no cross
        assert tr.topology(out) == tr.topology(g) and converged
        return
    assert np.array_equal(out, g) and (iterations, removed, converged) == (1, 0, True)
    assert int(tr.thin(g, tr.KERNEL)[0].sum()) == 1                     # ... and the kernel takes it for what it is, a tree


def test_the_counts_of_some_configurations():
    bit = {off: 1 << k for k, off in enumerate(tr.OFFSETS)}
    assert (tr.N26, tr.N18, tr.N6) == (0x7ffdfff, sum(bit[o] for o in tr.OFFSETS if 1 <= sum(map(abs, o)) <= 2), sum(bit[o] for o in tr.OFFSETS if sum(map(abs, o)) == 1))
    cases = {0: (0, 1), tr.N26: (1, 0), bit[(0, 0, 1)]: (1, 1), bit[(0, 0, 1)] | bit[(0, 0, -1)]: (2, 1),
             bit[(1, 1, 1)] | bit[(-1, -1, -1)]: (2, 1), tr.N26 & ~bit[(0, 0, 1)] & ~bit[(0, 0, -1)]: (1, 2),
             tr.N26 & ~bit[(1, 1, 1)]: (1, 0)}
    for cfg, (t26, t6) in cases.items():
        assert (int(tr.T26([cfg])[0]), int(tr.T6([cfg])[0])) == (t26, t6), hex(cfg)
    L = thin_host.library()
    for cfg, (t26, t6) in cases.items():
        assert (L.tc_T26(cfg), L.tc_T6(cfg), L.tc_simple(cfg)) == (t26, t6, int(t26 == 1 and t6 == 1)), hex(cfg)


# ---- the product's routines, compiled for the CPU, against the restatement ------------------------------------------------------------------
def test_header_counts_equal_the_restatements_on_random_configurations():
    rng = np.random.default_rng(26)
    dense = rng.integers(0, 1 << 27, 60000, dtype=np.uint32)
    sparse = dense & rng.integers(0, 1 << 27, 60000, dtype=np.uint32) & rng.integers(0, 1 << 27, 60000, dtype=np.uint32)
    cfg = np.concatenate([dense, sparse, ~sparse]) & np.uint32(tr.N26)
    is_simple, kept, t26, t6 = thin_host.decide(cfg)
    assert np.array_equal(t26, tr.T26(cfg)) and np.array_equal(t6, tr.T6(cfg))
    assert np.array_equal(is_simple, tr.simple(cfg)) and np.array_equal(kept, tr.popcount(cfg) == 1)
    assert 0.05 < is_simple.mean() < 0.95


def test_a_row_window_crosses_the_word_boundaries():
    L = thin_host.library()
    rng = np.random.default_rng(63)
    for _ in range(200):
        prev, cur, nxt = (int(v) for v in rng.integers(0, 1 << 63, 3, dtype=np.uint64) * 2 + rng.integers(0, 2, 3, dtype=np.uint64))
        row = prev | (cur << 64) | (nxt << 128)
        for b in (0, 1, 31, 61, 62, 63):
            assert L.tc_three(prev, cur, nxt, b) == (row >> (64 + b - 1)) & 7, (hex(prev), hex(cur), hex(nxt), b)


def check_product(g, what_for, limits=(0, 1, 2)):
    for kind in tr.KINDS:
        for limit in limits:
            want = tr.thin(g, kind, limit)
            for eight in (True, False) if g.shape[0] % 8 == 0 else (False,):        # the 8-byte path of pack and write-back (N % 8 == 0), and the byte path
                got = thin_host.thin(g, kind, limit, eight)
                assert got[0].dtype == np.uint8 and np.array_equal(got[0], want[0]), (what_for, kind, limit, eight)
                assert got[1:] == want[1:], (what_for, kind, limit, eight, got[1:], want[1:])


@pytest.mark.parametrize("N", SIDES)
def test_product_routines_equal_restatement_on_the_shapes(N):
    for what, g in ts.shapes(N):
        check_product(g, (N, what))


@pytest.mark.parametrize("N", gs.SWEEP + gs.WIDE)
def test_product_routines_equal_restatement_at_every_side(N):
    """every even side to 72 and the three longer rows.  The restatement of "all 0xFF" takes 1.4 s at side 72, 2.5 s at 130 and 5 s at 194 per
    kind here, "ends" 0.4 s, 0.6 s and 1.1 s for KERNEL, so the longer rows are in (with the product's own runs a case takes 10 s at 126 and 130,
    19 s at 194).  "random 0.3" runs at every side to 72: 2.3 s for both kinds at 72 (every distinct neighbourhood is decided once), a case there
    9 s.  "random 0.6" takes 1 s at 32 and 6 s and more from 66 on, so it stops at 32 -- and runs once more at 66, two words with N % 8 != 0,
    to the fixed point only (that case takes 18 s): tests/test_gpu_thin_sides.py takes the host library's word for that grid above 32."""
    names = ("all 0xFF", "ends") if N in gs.WIDE else ("all 0xFF", "ends", "hollow box", "random 0.3") + (("random 0.6",) if N <= 32 or N == 66 else ())
    for what, g in gs.grids(N, names):
        check_product(g, (N, what), limits=(0,) if N in gs.WIDE or (what, N) == ("random 0.6", 66) else (0, 2))


def test_batches_split_a_bounded_run():
    L = thin_host.library()
    assert (L.tc_rounds_default(), L.tc_rounds_max(), L.tc_max_n()) == (L.tc_rounds_default(), 64, 2048) and 1 <= L.tc_rounds_default() <= 64
    assert [L.tc_batch(r, left) for r, left in ((8, 0), (8, 3), (8, 8), (8, 9), (0, 0), (65, 0), (64, 100))] == [8, 3, 8, 8, 1, 64, 64]


# ---- the order --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", (6, 8, 16))
def test_the_subfield_order_matters(N):
    """thinning the x-mirrored grid and mirroring back visits the subfields in another order: other bytes for the random grids, so byte equality
    with the device elsewhere proves the order.  The hollow box is symmetric enough not to care."""
    for what, g in gs.grids(N, ("random 0.6", "random 0.3", "hollow box")):
        for kind in tr.KINDS:
            straight = tr.thin(g, kind)[0]
            mirrored = tr.thin(g[:, :, ::-1], kind)[0][:, :, ::-1]
            assert tr.topology(mirrored) == tr.topology(straight), (N, what, kind)
            if what == "hollow box":
                assert np.array_equal(straight, mirrored), (N, what, kind)
            else:
                assert not np.array_equal(straight, mirrored), (N, what, kind)
                assert np.array_equal(thin_host.thin(g, kind)[0], straight), (N, what, kind)


# ---- the boundary ------------------------------------------------------------------------------------------------------------------------
def test_header_declares_the_thin_entries(tmp_path):
    text = open(os.path.join(ROOT, "include", "dxv.h")).read()
    names = set(re.findall(r"DXV_API\s+[\w\s\*]+?\b(dxv_\w+)\s*\(", text))
    entries = {"dxv_thin_async", "dxv_thin", "dxv_thin_info"}
    assert entries <= names
    for phrase in ("Voxels outside the grid are EMPTY", "UNLIKE dxv_morph", "T26(p) == 1 && T6(p) == 1", "thinrounds 0..64"):
        assert phrase.lower() in text.lower(), phrase
    src = tmp_path / "use.c"
    src.write_text('#include "dxv.h"\n'
                   'int main(void) { dxv_ctx* c = 0; float ms = 0; uint32_t it = 0; uint64_t gone = 0; int conv = 0;\n'
                   '  int a[DXV_THIN_CURVE == 0 && DXV_THIN_KERNEL == 1 ? 1 : -1]; (void)a;\n'
                   '  return dxv_thin_async(c, DXV_THIN_CURVE, 0u) + dxv_thin(c, DXV_THIN_KERNEL, 3u) + dxv_thin_info(c, &ms, &it, &gone, &conv) + dxv_thin_info(c, 0, 0, 0, 0); }\n')
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), "-c", str(src),
                           "-o", str(tmp_path / "use.o")])
    from dxrvoxelizer_amd import _lib
    import dxrvoxelizer_amd as dxv
    version = int(re.search(r"#define DXV_API_VERSION (\d+)\b", text).group(1))
    assert _lib.API_VERSION == version and entries <= set(_lib.SYMBOLS)  # header and binding agree
    assert (dxv.THIN_CURVE, dxv.THIN_KERNEL) == tr.KINDS
    assert callable(dxv.Voxelizer.Thin) and callable(dxv.Voxelizer.thin_info)
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), "-x", "c++", "-"], check=True,
                   input=b'#include "dxv_voxelizer.hpp"\nint main() { Voxelizer v; float ms; uint32_t it; uint64_t gone; bool conv; '
                         b'return v.Thin(DXV_THIN_CURVE) + v.Thin(DXV_THIN_KERNEL, 3, false) + v.ThinInfo(ms, it, gone, conv); }\n')
