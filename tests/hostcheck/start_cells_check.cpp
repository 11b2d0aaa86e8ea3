// start_cells_check.cpp -- TEST-ONLY: the lists' start cells (dxv_dirmap.h: dm_start_cell, dm_start_cell_begin) on the CPU.
// One translation unit with start_table_check.cpp (and through it hostcheck.cpp): the host scene, its lists and its table are used as
// they stand, plus:
//   sc_cells        the start cells of the scene's lists, cell for cell what dirmap_starts makes on the device (the same functions)
//   sc_probe        every texel, every probe radius of st_probe: where the NEW body begins its scan against the exact first entry
//   sc_voxelize     grids through the brick kernels' bodies: canonical cells without a table, canonical cells and the table's word (the
//                   body of before), start cells (the body the table kernels run now), and the brick-box body (trace_reference_lists)
//   sc_round_stats  st_round_stats with the start of either body (tools/round_stats.py --cells)
// Never linked into libdxv.so.
#include "start_table_check.cpp"

// one voxel of a brick kernel of voxelize_lists.hip behind the brick's set-up, like voxel_listed (hostcheck.cpp), with the view the
// kernel of that FORM makes: 0 = _plain, 1 = the table kernels of before (cell + word), 2 = the table kernels (start cell)
template <int HITLDS, int FORM>
static uint8_t voxel_listed_form(const SceneView& sc, uint32_t N, uint32_t ix, uint32_t iy, uint32_t iz, uint32_t& texel)
{
    int32_t column[HITLDS == 1 ? 20 : 16];
    const StridedStack stk{column, 1};
    Ray r;
    ray_origin(N, ix, iy, iz, r.ox, r.oy, r.oz);
    const DirMapView dm{static_cast<const DirCell*>(sc.dmCells), static_cast<const DirEntry*>(sc.dmEntries), sc.dmR, sc.dmCoop, FORM == 1 ? sc.dmStarts : nullptr,
                        FORM == 2 ? static_cast<const DirCell*>(sc.dmStartCells) : nullptr};
    DirRayStart start = dm_ray_start<FORM>(r.ox, r.oy, r.oz, dm);
    if (origin_leaves_root(r.ox, r.oy, r.oz, sc.rootLo, sc.rootHi)) start.live = false;
    Hit best;
    float bestDet = 1.0f;
    trace_reference_dm_from<StridedStack, 0, HITLDS, FORM>(r, dm, start, sc.triPos, stk, 16, best, bestDet);
    texel = 0;
    return HITLDS == 1 ? shade_reference_lds(sc, r, best.leaf, stk, 16, &texel) : shade_reference_again(sc, r, best.leaf);
}

extern "C" {

__attribute__((visibility("default"))) uint32_t sc_direct(void) { return kDmStartCellDirect; }

__attribute__((visibility("default"))) void sc_cells_raw(const void* cells, uint32_t ncells, const void* entries, void* out)
{
    const DirCell* c = static_cast<const DirCell*>(cells);
    const DirEntry* e = static_cast<const DirEntry*>(entries);
    DirCell* o = static_cast<DirCell*>(out);
    for (uint32_t k = 0; k < ncells; ++k) o[k] = dm_start_cell(c[k], dm_start_word(c[k], e + c[k].begin));
}
__attribute__((visibility("default"))) void sc_cells(void* p, void* out)
{
    HcScene* s = static_cast<HcScene*>(p);
    DirCell* o = static_cast<DirCell*>(out);
#pragma omp parallel for schedule(static, 1024)
    for (int64_t c = 0; c < (int64_t)s->dmCells.size(); ++c) o[c] = dm_start_cell(s->dmCells[c], dm_start_word(s->dmCells[c], s->dmEntries.data() + s->dmCells[c].begin));
}

// The probe radii of st_probe (every entry's far radius and the halfs next to it, the half below the first entry's, r1max), each as a ray's
// `near`, through dm_start_cell_begin with `live` decided as dm_ray_start decides it:
//   a live ray's scan must begin inside the list and at most at the exact first entry with !(r1 < near)   -> out[1] counts later starts
//   a ray that is not live must begin at the list's end                                                    -> out[2]
// out[0] probes, out[3] texels, out[4] texels longer than `direct` (they search), out[5] the longest list, out[6] probes whose start is not
// entry 0, out[7] texel of the first failure + 1, out[8] search loads, out[9] probes whose start lies in front of the old body's (hints,
// search, table: canonical cells and `starts` given), out[10] probes whose start lies behind it
__attribute__((visibility("default"))) void sc_probe_raw(const void* startCells, const void* cells, const uint32_t* starts, uint32_t ncells, const void* entriesIn,
                                                         uint32_t direct, uint64_t* out)
{
    const DirCell* sc = static_cast<const DirCell*>(startCells);
    const DirCell* canon = static_cast<const DirCell*>(cells);
    const DirEntry* entries = static_cast<const DirEntry*>(entriesIn);
    uint64_t probes = 0, late = 0, dead = 0, texels = 0, big = 0, moved = 0, longest = 0, firstBad = 0, loads = 0, earlier = 0, later = 0;
#pragma omp parallel for schedule(dynamic, 256) reduction(+ : probes, late, dead, texels, big, moved, loads, earlier, later) reduction(max : longest, firstBad)
    for (int64_t c = 0; c < (int64_t)ncells; ++c) {
        const DirCell cell = sc[c];
        if (!cell.count) continue;
        ++texels;
        if (cell.count > direct) ++big;
        if (cell.count > longest) longest = cell.count;
        const DirEntry* list = entries + cell.begin;
        auto probe = [&](uint32_t key) {
            if (key < 0x0400u || key > 0x7bffu) return;
            const float near = half_bits_to_float(key);
            const bool live = !(half_bits_to_float(cell.r1max) < near);
            uint32_t n = 0;
            const uint32_t got = dm_start_cell_begin(cell, entries, live, near, direct, &n) - cell.begin;
            loads += n;
            ++probes;
            bool bad = false;
            if (!live) { if (got != cell.count) { ++dead; bad = true; } }
            else {
                uint32_t exact = 0;
                while (exact < cell.count && dm_entry_r1(list[exact]) < near) ++exact;
                if (got > exact || got >= cell.count) { ++late; bad = true; }
                if (got) ++moved;
                if (canon && starts) {                                  // the body of before: hints, search, table
                    const DirCell cc = canon[c];
                    uint32_t i = 0, hi = cc.count;
                    if (hi - i > 8u) {
                        const uint32_t mid = i + ((hi - i) >> 1);
                        const bool right = half_bits_to_float(cc.q2) < near;
                        const float q = half_bits_to_float(right ? cc.q3 : cc.q1);
                        if (right) i = mid + 1u; else hi = mid;
                        if (hi - i > 8u) { const uint32_t mid2 = i + ((hi - i) >> 1); if (q < near) i = mid2 + 1u; else hi = mid2; }
                    }
                    while (hi - i > 8u) { const uint32_t mid = i + ((hi - i) >> 1); if (dm_entry_r1(list[mid]) < near) i = mid + 1u; else hi = mid; }
                    const uint32_t from = dm_start_offset(starts[c], cc.count, cc.r1max, near);
                    if (from > i) i = from;
                    if (got < i) ++earlier;
                    if (got > i) ++later;
                }
            }
            if (bad && (uint64_t)c + 1 > firstBad) firstBad = (uint64_t)c + 1;
        };
        const uint32_t k0 = dm_entry_key(list[0]), top = cell.r1max;
        if (k0 > 0u) probe(k0 - 1u);
        probe(top); probe(top + 1u);
        for (uint32_t k = 0; k < cell.count; ++k) {
            const uint32_t ke = dm_entry_key(list[k]);
            if (k && ke == dm_entry_key(list[k - 1])) continue;
            if (ke > 0u) probe(ke - 1u);
            probe(ke); probe(ke + 1u);
        }
    }
    out[0] = probes; out[1] = late; out[2] = dead; out[3] = texels; out[4] = big; out[5] = longest; out[6] = moved; out[7] = firstBad; out[8] = loads;
    out[9] = earlier; out[10] = later;
}
__attribute__((visibility("default"))) void sc_probe(void* p, const void* startCells, const uint32_t* starts, uint32_t direct, uint64_t* out)
{
    HcScene* s = static_cast<HcScene*>(p);
    sc_probe_raw(startCells, s->dmCells.data(), starts, (uint32_t)s->dmCells.size(), s->dmEntries.data(), direct, out);
}

// grids (and the texel image) through the kernels' bodies.  form 0 / 1 / 2: the brick kernels' body (voxel_listed_form) without a table, with
// the table's word beside the canonical cell, with start cells; form 3: the brick-box body (voxel_reference<4>: trace_reference_lists) with
// whatever of starts / startCells is given -- it reads start cells where it has them.  hitlds as in st_voxelize (forms 0 .. 2).
__attribute__((visibility("default"))) int sc_voxelize(void* p, uint32_t N, int hitlds, int form, const uint32_t* starts, const void* startCells, uint8_t* out, uint32_t* texels)
{
    HcScene* s = static_cast<HcScene*>(p);
    if (!s->dmR || (hitlds != 1 && hitlds != 2) || (hitlds == 2 && texels && form != 3) || form < 0 || form > 3) return -1;
    if ((form == 1 && !starts) || (form == 2 && !startCells)) return -1;
    SceneView sc{s->nodes32.data(), s->triPos.data(), s->triNrm.data(), {0, 0, 0}, {0, 0, 0}, s->nodes64.data(),
                 s->dmCells.data(), s->dmEntries.data(), s->dmR};
    sc.dmStarts = starts; sc.dmStartCells = startCells;
    const float* w = reinterpret_cast<const float*>(&s->nodes[0]);
    for (int a = 0; a < 3; ++a) { sc.rootLo[a] = min_(w[a], w[6 + a]); sc.rootHi[a] = max_(w[3 + a], w[9 + a]); }
#pragma omp parallel for schedule(dynamic, 4)
    for (int64_t row = 0; row < (int64_t)N * N; ++row) {
        const uint32_t iz = (uint32_t)(row / N), iy = (uint32_t)(row % N);
        for (uint32_t ix = 0; ix < N; ++ix) {
            const size_t id = ((size_t)iz * N + iy) * N + ix;
            uint32_t texel = 0;
            uint8_t occ;
            if (form == 3) {
                int32_t column[16];
                const StridedStack stk{column, 1};
                bool overflow = false;
                occ = voxel_reference<4>(sc, N, ix, iy, iz, stk, 16, texels ? &texel : nullptr, overflow);
            }
            else if (hitlds == 1) occ = form == 0 ? voxel_listed_form<1, 0>(sc, N, ix, iy, iz, texel) : form == 1 ? voxel_listed_form<1, 1>(sc, N, ix, iy, iz, texel) : voxel_listed_form<1, 2>(sc, N, ix, iy, iz, texel);
            else occ = form == 0 ? voxel_listed_form<2, 0>(sc, N, ix, iy, iz, texel) : form == 1 ? voxel_listed_form<2, 1>(sc, N, ix, iy, iz, texel) : voxel_listed_form<2, 2>(sc, N, ix, iy, iz, texel);
            out[id] = occ;
            if (texels) texels[id] = texel;
        }
    }
    return 0;
}

// st_round_stats (start_table_check.cpp: the lockstep replay of the device loop per 4^3 brick; out[] as there) with the start of a ray's
// scan made by the body asked for: startCells NULL -- hints, search and the table's word from `starts` (the replay of st_round_stats itself,
// number for number); else dm_start_cell_begin on the start cell, lists of up to `direct` entries without a search.
__attribute__((visibility("default"))) void sc_round_stats(void* p, uint32_t N, uint32_t bstep, const uint32_t* starts, const void* startCellsIn, uint32_t direct, int coopOn,
                                                           uint64_t* out)
{
    HcScene* s = static_cast<HcScene*>(p);
    float rootLo[3], rootHi[3];
    {
        const float* w = reinterpret_cast<const float*>(&s->nodes[0]);
        for (int a = 0; a < 3; ++a) { rootLo[a] = min_(w[a], w[6 + a]); rootHi[a] = max_(w[3 + a], w[9 + a]); }
    }
    const DirMapView dm{s->dmCells.data(), s->dmEntries.data(), s->dmR, 0u, starts, static_cast<const DirCell*>(startCellsIn)};
    const TriPos* tris = s->triPos.data();
    const uint32_t nb = N / 4;
    const int cap = 16;
    uint64_t o[14] = {0};
#pragma omp parallel for schedule(dynamic, 1) reduction(+ : o[:14])
    for (int64_t bzi = 0; bzi < (int64_t)nb; bzi += bstep) {
        for (uint32_t byi = 0; byi < nb; ++byi) for (uint32_t bxi = 0; bxi < nb; ++bxi) {
            struct Lane { Ray r; float rho, near, step, bound, bestT; int32_t bestLeaf; uint32_t i, end, rc; DirRayLocal loc; int qn; int32_t q[16]; };
            Lane ln[64];
            bool anyLive = false;
            uint32_t searchMax = 0;
            for (int t = 0; t < 64; ++t) {
                Lane& l = ln[t];
                const uint32_t ix = bxi * 4 + t % 4, iy = byi * 4 + (t / 4) % 4, iz = (uint32_t)bzi * 4 + t / 16;
                ray_origin(N, ix, iy, iz, l.r.ox, l.r.oy, l.r.oz);
                DirRayStart st = dm_ray_start<3>(l.r.ox, l.r.oy, l.r.oz, dm);
                if (origin_leaves_root(l.r.ox, l.r.oy, l.r.oz, rootLo, rootHi)) st.live = false;
                if (st.live) { anyLive = true; ++o[13]; }
                const DirCell cell = st.cell;
                l.rho = st.rho; l.near = st.near;
                l.end = cell.begin + cell.count;
                uint32_t i = cell.begin, hi = l.end, loads = 0;
                if (dm.startCells) {
                    i = dm_start_cell_begin(cell, dm.entries, st.live, l.near, direct, &loads);
                    if (st.live && i > cell.begin) ++o[12];
                } else {
                    if (!st.live) i = hi;
                    if (hi - i > 8u) {
                        const uint32_t mid = i + ((hi - i) >> 1);
                        const bool right = half_bits_to_float(cell.q2) < l.near;
                        const float q = half_bits_to_float(right ? cell.q3 : cell.q1);
                        if (right) i = mid + 1u; else hi = mid;
                        if (hi - i > 8u) { const uint32_t mid2 = i + ((hi - i) >> 1); if (q < l.near) i = mid2 + 1u; else hi = mid2; }
                    }
                    while (hi - i > 8u) { const uint32_t mid = i + ((hi - i) >> 1); ++loads; if (dm_entry_r1(dm.entries[mid]) < l.near) i = mid + 1u; else hi = mid; }
                    const uint32_t from = cell.begin + dm_start_offset(st.startWord, cell.count, cell.r1max, l.near);
                    if (from > i) { i = from; ++o[12]; }
                }
                o[5] += loads;
                if (loads > searchMax) searchMax = loads;
                l.i = i; l.qn = 0; l.bestT = kTMax; l.bestLeaf = -1;
                l.step = dm_stop_step(half_bits_to_float(cell.thick));
                l.loc = dm_ray_local(st.cx, st.cy);
                l.bound = (l.rho + l.bestT) * 1.001f + 1e-4f;
                l.rc = dm_radial_word(l.near, l.bound);
            }
            if (!anyLive) continue;
            ++o[0]; o[4] += searchMax;
            bool scanned = false;
            auto push = [&](Lane& l, const DirEntry& e) { l.q[2 * l.qn] = (int32_t)dm_entry_tri(e); l.q[2 * l.qn + 1] = (int32_t)e.rr; ++l.qn; ++o[9]; };
            for (;;) {
                bool coop = false;
                int nscan = 0, L = -1;
                for (int t = 0; t < 64; ++t) if (ln[t].i < ln[t].end) { if (L < 0) L = t; ++nscan; }
                if (nscan) scanned = true;
                if (coopOn && nscan != 0 && nscan <= (int)kDmCoopLanes && ln[L].end - ln[L].i >= kDmCoopMin) {
                    Lane& l = ln[L];
                    const uint32_t iL = l.i, endL = l.end, width = 64u;
                    uint32_t stopRank = 64u;
                    for (uint32_t k = 0; k < width && iL + k < endL; ++k) if (dm_stop_radius(dm.entries[iL + k], l.step) > l.bound) { stopRank = k; break; }
                    uint32_t next = stopRank < 64u ? endL : (iL + width < endL ? iL + width : endL);
                    for (uint32_t k = 0; k < width && iL + k < endL && k < stopRank; ++k) {
                        ++o[8];
                        if (!dm_local_pass(dm.entries[iL + k], l.loc, l.rc)) continue;
                        if (2 * (l.qn + 1) > cap) { next = iL + k; break; }
                        push(l, dm.entries[iL + k]);
                    }
                    l.i = next;
                    coop = true;
                    ++o[10]; ++o[2]; ++o[3];
                }
                if (!coop && nscan) {
                    bool wide = false;
                    for (int t = 0; t < 64; ++t) if (ln[t].i < ln[t].end && ln[t].i + 2u <= ln[t].end - 1u) wide = true;
                    ++o[2]; o[3] += wide ? 4u : 2u;
                    for (int t = 0; t < 64; ++t) {
                        Lane& l = ln[t];
                        if (!(l.i < l.end)) continue;
                        const uint32_t last = l.end - 1u;
                        const DirEntry* e = dm.entries + l.i;
                        if (dm_stop_radius(e[0], l.step) > l.bound) { l.i = l.end; continue; }
                        const uint32_t look = wide ? 4u : 2u;
                        for (uint32_t k = 0; k < look; ++k) {
                            if (l.i + k > last) break;
                            ++o[8];
                            if (dm_local_pass(e[k], l.loc, l.rc)) push(l, e[k]);
                        }
                        l.i += 4u;
                    }
                }
                bool scanning = false, full = false;
                for (int t = 0; t < 64; ++t) { if (ln[t].i < ln[t].end) scanning = true; if (2 * (ln[t].qn + 4) > cap) full = true; }
                ++o[1];
                if (scanning && !full) continue;
                ++o[7];
                int k[64] = {0};
                for (int t = 0; t < 64; ++t) if (ln[t].qn) { finish_ray_reference(ln[t].r, ln[t].rho); ray_shear_finished(ln[t].r); }
                for (;;) {
                    bool any = false;
                    for (int t = 0; t < 64; ++t) {
                        Lane& l = ln[t];
                        while (k[t] < l.qn && (((uint32_t)l.q[2 * k[t] + 1] - l.rc) & 0x00008000u) == 0u) ++k[t];
                        if (k[t] < l.qn) any = true;
                    }
                    if (!any) break;
                    for (int t = 0; t < 64; ++t) {
                        Lane& l = ln[t];
                        if (!(k[t] < l.qn)) continue;
                        leaf_reference_min(l.r, tris, l.q[2 * k[t]], l.bestT, l.bestLeaf);
                        l.bound = (l.rho + l.bestT) * 1.001f + 1e-4f;
                        l.rc = dm_radial_word(l.near, l.bound);
                        ++k[t];
                    }
                    ++o[6];
                }
                for (int t = 0; t < 64; ++t) ln[t].qn = 0;
                if (!scanning) break;
            }
            if (scanned) ++o[11];
        }
    }
    for (int i = 0; i < 14; ++i) out[i] = o[i];
}

} // extern "C"
