// start_table_check.cpp -- TEST-ONLY: the lists' start table (dxv_dirmap.h: dm_start_word, dm_start_offset) on the CPU.
// One translation unit with hostcheck.cpp -- its host scene, its host-built lists (hc_dirmap_build) and the brick kernels' own
// bodies (voxel_listed) are used as they stand -- plus:
//   st_table        the table of the scene's lists, word for word what dirmap_starts makes on the device (the same function)
//   st_probe        every texel, every probe radius: the table's start against the exact first entry and the bucket's first entry
//   st_voxelize     grids through the kernels' bodies with a table (or without: starts = NULL)
//   st_round_stats  a lockstep replay of trace_reference_dm_from per 4 x 4 x 4 brick: what a wave of the lists kernel issues
//                   (tools/round_stats.py)
// Never linked into libdxv.so.
#include "hostcheck.cpp"

extern "C" {

__attribute__((visibility("default"))) void st_table(void* p, uint32_t* out)
{
    HcScene* s = static_cast<HcScene*>(p);
#pragma omp parallel for schedule(static, 1024)
    for (int64_t c = 0; c < (int64_t)s->dmCells.size(); ++c) out[c] = dm_start_word(s->dmCells[c], s->dmEntries.data() + s->dmCells[c].begin);
}

__attribute__((visibility("default"))) uint32_t st_buckets(void) { return kDmStartBuckets; }
__attribute__((visibility("default"))) uint32_t st_offset(uint32_t word, uint32_t count, uint32_t top, float near) { return dm_start_offset(word, count, top, near); }

// Probe radii of a texel: every entry's far radius and the halfs next to it on both sides, the half below the first entry's, and r1max.
// For each, with near = that half's value: the table's start must be
//   (a) at most the exact first entry with !(r1 < near)                                    -> out[1] counts starts behind it
//   (b) at least the first entry of the ray's bucket, rounded down to a multiple of `unit` -> out[2] counts starts in front of it
// out[0] probes, out[3] texels, out[4] texels of more than 255 entries (unit > 1), out[5] the longest list, out[6] probes whose
// start is not entry 0, out[7] texel of the first failure + 1
static void probe_lists(const DirCell* cells, size_t ncells, const DirEntry* entries, const uint32_t* starts, uint64_t* out)
{
    uint64_t probes = 0, late = 0, early = 0, texels = 0, big = 0, moved = 0, longest = 0, firstBad = 0;
#pragma omp parallel for schedule(dynamic, 256) reduction(+ : probes, late, early, texels, big, moved) reduction(max : longest, firstBad)
    for (int64_t c = 0; c < (int64_t)ncells; ++c) {
        const DirCell cell = cells[c];
        if (!cell.count) { if (starts[c] != 0u) { ++early; firstBad = (uint64_t)c + 1; } continue; }
        ++texels;
        if (cell.count > 255u) ++big;
        if (cell.count > longest) longest = cell.count;
        const DirEntry* list = entries + cell.begin;
        const uint32_t word = starts[c], sh = word & 15u, top = cell.r1max, unit = dm_start_unit(cell.count);
        auto probe = [&](uint32_t key) {
            if (key < 0x0400u || key > 0x7bffu) return;                 // (outside the halfs' normal range: no ray starts there)
            const float near = half_bits_to_float(key);
            const uint32_t got = dm_start_offset(word, cell.count, top, near);
            uint32_t exact = 0;
            while (exact < cell.count && dm_entry_r1(list[exact]) < near) ++exact;
            ++probes;
            if (got) ++moved;
            bool bad = got > exact;
            if (bad) ++late;
            // the ray's bucket: the first entry whose bucket is not greater, rounded down by unit (key > top: no skip asked for)
            uint32_t want = 0;
            if (key <= top) {
                const uint32_t d = (top - key) >> sh;
                if (d < kDmStartBuckets - 1u) { while (want < cell.count && dm_start_bucket(top, sh, dm_entry_key(list[want])) > d) ++want; }
                want = want / unit * unit;
            }
            if (got < want) { ++early; bad = true; }
            if (bad && (uint64_t)c + 1 > firstBad) firstBad = (uint64_t)c + 1;
        };
        const uint32_t k0 = dm_entry_key(list[0]);
        if (k0 > 0u) probe(k0 - 1u);
        probe(top);
        for (uint32_t k = 0; k < cell.count; ++k) {
            const uint32_t ke = dm_entry_key(list[k]);
            if (k && ke == dm_entry_key(list[k - 1])) continue;
            if (ke > 0u) probe(ke - 1u);
            probe(ke); probe(ke + 1u);
        }
    }
    out[0] = probes; out[1] = late; out[2] = early; out[3] = texels; out[4] = big; out[5] = longest; out[6] = moved; out[7] = firstBad;
}
__attribute__((visibility("default"))) void st_probe(void* p, const uint32_t* starts, uint64_t* out)
{
    HcScene* s = static_cast<HcScene*>(p);
    probe_lists(s->dmCells.data(), s->dmCells.size(), s->dmEntries.data(), starts, out);
}
// ... and for lists the caller made up (cells and entries as the device holds them): their table into `starts`, then the probes
__attribute__((visibility("default"))) void st_probe_raw(const void* cells, uint32_t ncells, const void* entries, uint32_t* starts, uint64_t* out)
{
    const DirCell* c = static_cast<const DirCell*>(cells);
    const DirEntry* e = static_cast<const DirEntry*>(entries);
    for (uint32_t k = 0; k < ncells; ++k) starts[k] = dm_start_word(c[k], e + c[k].begin);
    probe_lists(c, ncells, e, starts, out);
}

// grids (and the texel image) through the brick kernels' own bodies: hitlds 1 = k_voxelize_listed<true>, 2 = the kernels with the texel
// image off; starts: a table for the scene's lists, or NULL
__attribute__((visibility("default"))) int st_voxelize(void* p, uint32_t N, int hitlds, const uint32_t* starts, uint8_t* out, uint32_t* texels)
{
    HcScene* s = static_cast<HcScene*>(p);
    if (!s->dmR || (hitlds != 1 && hitlds != 2) || (hitlds == 2 && texels)) return -1;
    SceneView sc{s->nodes32.data(), s->triPos.data(), s->triNrm.data(), {0, 0, 0}, {0, 0, 0}, s->nodes64.data(),
                 s->dmCells.data(), s->dmEntries.data(), s->dmR};
    sc.dmStarts = starts;
    const float* w = reinterpret_cast<const float*>(&s->nodes[0]);
    for (int a = 0; a < 3; ++a) { sc.rootLo[a] = min_(w[a], w[6 + a]); sc.rootHi[a] = max_(w[3 + a], w[9 + a]); }
#pragma omp parallel for schedule(dynamic, 4)
    for (int64_t row = 0; row < (int64_t)N * N; ++row) {
        const uint32_t iz = (uint32_t)(row / N), iy = (uint32_t)(row % N);
        for (uint32_t ix = 0; ix < N; ++ix) {
            const size_t id = ((size_t)iz * N + iy) * N + ix;
            uint32_t texel = 0;
            out[id] = hitlds == 1 ? voxel_listed<1>(sc, N, ix, iy, iz, texel) : voxel_listed<2>(sc, N, ix, iy, iz, texel);
            if (texels) texels[id] = texel;
        }
    }
    return 0;
}

// Lockstep replay of trace_reference_dm_from (HITLDS 2, the queue of 16 words, coop as given) for the 64 rays of every 4^3 brick of
// every bstep-th brick layer: the control flow of the device loop with the product's own functions for every decision -- dm_ray_start,
// the hint steps, the search loop, dm_start_offset, the 4-entry rounds with the `wide` vote, the cooperative round, the flush rule,
// the triangle rounds.  Bricks counted: those with a live ray (the device's queue holds a few more, whose one round finds nothing).
// out[0] bricks, [1] scan rounds as the device counts them (loop iterations), [2] scan rounds that loaded, [3] scan load instructions,
// [4] search load instructions (the longest lane's), [5] search loads of all lanes, [6] triangle rounds, [7] flushes, [8] entries looked
// at, [9] entries that passed, [10] cooperative rounds, [11] bricks that scan at all, [12] rays whose start the table moved, [13] live rays
__attribute__((visibility("default"))) void st_round_stats(void* p, uint32_t N, uint32_t bstep, const uint32_t* starts, int coopOn, uint64_t* out)
{
    HcScene* s = static_cast<HcScene*>(p);
    float rootLo[3], rootHi[3];
    {
        const float* w = reinterpret_cast<const float*>(&s->nodes[0]);
        for (int a = 0; a < 3; ++a) { rootLo[a] = min_(w[a], w[6 + a]); rootHi[a] = max_(w[3 + a], w[9 + a]); }
    }
    const DirMapView dm{s->dmCells.data(), s->dmEntries.data(), s->dmR, 0u, starts};
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
                DirRayStart st = dm_ray_start(l.r.ox, l.r.oy, l.r.oz, dm);
                if (origin_leaves_root(l.r.ox, l.r.oy, l.r.oz, rootLo, rootHi)) st.live = false;
                if (st.live) { anyLive = true; ++o[13]; }
                const DirCell cell = st.cell;
                l.rho = st.rho; l.near = st.near;
                l.end = cell.begin + cell.count;
                uint32_t i = cell.begin, hi = l.end, loads = 0;
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
