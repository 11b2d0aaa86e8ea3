// filter_check.cpp -- TEST-ONLY: what the lists' integer filter (dxv_dirmap.h: dm_local_pass -- box, radial range, ONE edge) lets through to
// the triangle step, and what of that finds nothing.  One translation unit with start_table_check.cpp (and through it hostcheck.cpp): the
// host scene, the host-built lists and the start table are used as they stand, plus:
//   fc_filter_stats  the lockstep replay of st_round_stats (the same control flow, the product's own functions for every decision) with
//                    every triangle test counted and classified, and optionally a PERFECT filter in place of the shipped one -- the floor
//                    (tools/filter_stats.py)
//   fc_edge_census   entries of the lists, and entries that carry no edge
//   fc_edge_cells    the edge term of an entry against all 128 x 128 cells of its texel, beside the real-valued dilated edge functions of
//                    the record (tests/test_edge_centre.py)
// Never linked into libdxv.so.
#include "start_table_check.cpp"

namespace {

// Does the line through the centre with the ray's direction pass through the triangle?  Exact enough to classify a miss: double
// throughout, barycentrics of the line's point in the triangle's plane.  Returns min(b0, b1, b2) (>= 0: through the triangle; the
// more negative, the farther outside, in units of the triangle's heights); a line in the triangle's plane counts as far outside.
double line_min_barycentric(const Ray& r, const TriPos& tp)
{
    const double d[3] = {r.ox, r.oy, r.oz};
    const double a[3] = {tp.v0.x, tp.v0.y, tp.v0.z}, b[3] = {tp.v1.x, tp.v1.y, tp.v1.z}, c[3] = {tp.v2.x, tp.v2.y, tp.v2.z};
    const double e1[3] = {b[0] - a[0], b[1] - a[1], b[2] - a[2]}, e2[3] = {c[0] - a[0], c[1] - a[1], c[2] - a[2]};
    const double n[3] = {e1[1] * e2[2] - e1[2] * e2[1], e1[2] * e2[0] - e1[0] * e2[2], e1[0] * e2[1] - e1[1] * e2[0]};
    const double nd = n[0] * d[0] + n[1] * d[1] + n[2] * d[2], na = n[0] * a[0] + n[1] * a[1] + n[2] * a[2];
    const double nn = n[0] * n[0] + n[1] * n[1] + n[2] * n[2];
    if (!(nd * nd > 1e-30 * nn * (d[0] * d[0] + d[1] * d[1] + d[2] * d[2])) || !(nn > 0.0)) return -1e30;
    const double s = na / nd;
    const double p[3] = {s * d[0] - a[0], s * d[1] - a[1], s * d[2] - a[2]};
    // p = b1 e1 + b2 e2 in the plane: b1 = n . (p x e2) / nn, b2 = n . (e1 x p) / nn
    const double pxe2[3] = {p[1] * e2[2] - p[2] * e2[1], p[2] * e2[0] - p[0] * e2[2], p[0] * e2[1] - p[1] * e2[0]};
    const double e1xp[3] = {e1[1] * p[2] - e1[2] * p[1], e1[2] * p[0] - e1[0] * p[2], e1[0] * p[1] - e1[1] * p[0]};
    const double b1 = (n[0] * pxe2[0] + n[1] * pxe2[1] + n[2] * pxe2[2]) / nn, b2 = (n[0] * e1xp[0] + n[1] * e1xp[1] + n[2] * e1xp[2]) / nn;
    const double b0 = 1.0 - b1 - b2;
    return b0 < b1 ? (b0 < b2 ? b0 : b2) : (b1 < b2 ? b1 : b2);
}

// the triangle step's own verdict on (ray, triangle), whatever the ray has found so far: the canonical test against no earlier hit
bool triangle_is_hit(Ray& r, const TriPos* tris, int32_t tri)
{
    float t = kTMax;
    int32_t leaf = -1;
    leaf_reference_min(r, tris, tri, t, leaf);
    return leaf != -1;
}

} // namespace

extern "C" {

constexpr int kFcOut = 20;
// The replay of st_round_stats (start_table_check.cpp; HITLDS 2, the queue of 16 words, the start table in `starts`), per 4 x 4 x 4 brick of
// every bstep-th brick layer, bricks with a live ray.  perfect != 0: an entry passes only if it passes dm_local_pass AND its triangle is hit
// by the ray (triangle_is_hit) -- no filter of any encoding does better.
// out[0] bricks, [1] scan rounds (loop iterations, as the device counts them), [2] triangle rounds, [3] triangle tests, [4] tests that hit,
// [5] misses whose line through the centre passes through the triangle (radial: the ray starts behind the point, or the hit is cut by the
// bound), [6 .. 10] lateral misses by -min barycentric: < 0.02, < 0.05, < 0.1, < 0.25, the rest, [11] entries looked at, [12] entries that
// passed, [13] flushes, [14] live rays, [15] the longest triangle step of a brick (rounds)
__attribute__((visibility("default"))) void fc_filter_stats(void* p, uint32_t N, uint32_t bstep, const uint32_t* starts, int coopOn, int perfect, uint64_t* out)
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
    uint64_t o[kFcOut] = {0};
    uint64_t longest = 0;
#pragma omp parallel for schedule(dynamic, 1) reduction(+ : o[:kFcOut]) reduction(max : longest)
    for (int64_t bzi = 0; bzi < (int64_t)nb; bzi += bstep) {
        for (uint32_t byi = 0; byi < nb; ++byi) for (uint32_t bxi = 0; bxi < nb; ++bxi) {
            struct Lane { Ray r, r0; float rho, near, step, bound, bestT; int32_t bestLeaf; uint32_t i, end, rc; DirRayLocal loc; int qn; int32_t q[16]; };
            Lane ln[64];
            bool anyLive = false;
            for (int t = 0; t < 64; ++t) {
                Lane& l = ln[t];
                const uint32_t ix = bxi * 4 + t % 4, iy = byi * 4 + (t / 4) % 4, iz = (uint32_t)bzi * 4 + t / 16;
                ray_origin(N, ix, iy, iz, l.r.ox, l.r.oy, l.r.oz);
                DirRayStart st = dm_ray_start(l.r.ox, l.r.oy, l.r.oz, dm);
                if (origin_leaves_root(l.r.ox, l.r.oy, l.r.oz, rootLo, rootHi)) st.live = false;
                if (st.live) { anyLive = true; ++o[14]; }
                const DirCell cell = st.cell;
                l.rho = st.rho; l.near = st.near;
                l.end = cell.begin + cell.count;
                uint32_t i = cell.begin, hi = l.end;
                if (!st.live) i = hi;
                if (hi - i > 8u) {
                    const uint32_t mid = i + ((hi - i) >> 1);
                    const bool right = half_bits_to_float(cell.q2) < l.near;
                    const float q = half_bits_to_float(right ? cell.q3 : cell.q1);
                    if (right) i = mid + 1u; else hi = mid;
                    if (hi - i > 8u) { const uint32_t mid2 = i + ((hi - i) >> 1); if (q < l.near) i = mid2 + 1u; else hi = mid2; }
                }
                while (hi - i > 8u) { const uint32_t mid = i + ((hi - i) >> 1); if (dm_entry_r1(dm.entries[mid]) < l.near) i = mid + 1u; else hi = mid; }
                const uint32_t from = cell.begin + dm_start_offset(st.startWord, cell.count, cell.r1max, l.near);
                if (from > i) i = from;
                l.i = i; l.qn = 0; l.bestT = kTMax; l.bestLeaf = -1;
                l.step = dm_stop_step(half_bits_to_float(cell.thick));
                l.loc = dm_ray_local(st.cx, st.cy);
                l.bound = (l.rho + l.bestT) * 1.001f + 1e-4f;
                l.rc = dm_radial_word(l.near, l.bound);
                // (the direction and the shear every triangle test of this ray uses, made once on a copy: the perfect filter asks before a flush)
                l.r0 = l.r;
                if (st.live) { finish_ray_reference(l.r0, l.rho); ray_shear_finished(l.r0); }
            }
            if (!anyLive) continue;
            ++o[0];
            uint64_t roundsHere = 0;
            auto pass = [&](Lane& l, const DirEntry& e) {
                if (!dm_local_pass(e, l.loc, l.rc)) return false;
                return !perfect || triangle_is_hit(l.r0, tris, (int32_t)dm_entry_tri(e));
            };
            auto push = [&](Lane& l, const DirEntry& e) { l.q[2 * l.qn] = (int32_t)dm_entry_tri(e); l.q[2 * l.qn + 1] = (int32_t)e.rr; ++l.qn; ++o[12]; };
            for (;;) {
                bool coop = false;
                int nscan = 0, L = -1;
                for (int t = 0; t < 64; ++t) if (ln[t].i < ln[t].end) { if (L < 0) L = t; ++nscan; }
                if (coopOn && nscan != 0 && nscan <= (int)kDmCoopLanes && ln[L].end - ln[L].i >= kDmCoopMin) {
                    Lane& l = ln[L];
                    const uint32_t iL = l.i, endL = l.end, width = 64u;
                    uint32_t stopRank = 64u;
                    for (uint32_t k = 0; k < width && iL + k < endL; ++k) if (dm_stop_radius(dm.entries[iL + k], l.step) > l.bound) { stopRank = k; break; }
                    uint32_t next = stopRank < 64u ? endL : (iL + width < endL ? iL + width : endL);
                    for (uint32_t k = 0; k < width && iL + k < endL && k < stopRank; ++k) {
                        ++o[11];
                        if (!pass(l, dm.entries[iL + k])) continue;
                        if (2 * (l.qn + 1) > cap) { next = iL + k; break; }
                        push(l, dm.entries[iL + k]);
                    }
                    l.i = next;
                    coop = true;
                }
                if (!coop && nscan) {
                    bool wide = false;
                    for (int t = 0; t < 64; ++t) if (ln[t].i < ln[t].end && ln[t].i + 2u <= ln[t].end - 1u) wide = true;
                    for (int t = 0; t < 64; ++t) {
                        Lane& l = ln[t];
                        if (!(l.i < l.end)) continue;
                        const uint32_t last = l.end - 1u;
                        const DirEntry* e = dm.entries + l.i;
                        if (dm_stop_radius(e[0], l.step) > l.bound) { l.i = l.end; continue; }
                        const uint32_t look = wide ? 4u : 2u;
                        for (uint32_t k = 0; k < look; ++k) {
                            if (l.i + k > last) break;
                            ++o[11];
                            if (pass(l, e[k])) push(l, e[k]);
                        }
                        l.i += 4u;
                    }
                }
                bool scanning = false, full = false;
                for (int t = 0; t < 64; ++t) { if (ln[t].i < ln[t].end) scanning = true; if (2 * (ln[t].qn + 4) > cap) full = true; }
                ++o[1];
                if (scanning && !full) continue;
                ++o[13];
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
                        const int32_t tri = l.q[2 * k[t]];
                        ++o[3];
                        if (triangle_is_hit(l.r, tris, tri)) ++o[4];
                        else {
                            const double mb = line_min_barycentric(l.r, load_tri(tris, tri));
                            if (mb >= 0.0) ++o[5];
                            else ++o[-mb < 0.02 ? 6 : -mb < 0.05 ? 7 : -mb < 0.1 ? 8 : -mb < 0.25 ? 9 : 10];
                        }
                        leaf_reference_min(l.r, tris, tri, l.bestT, l.bestLeaf);
                        l.bound = (l.rho + l.bestT) * 1.001f + 1e-4f;
                        l.rc = dm_radial_word(l.near, l.bound);
                        ++k[t];
                    }
                    ++o[2]; ++roundsHere;
                }
                for (int t = 0; t < 64; ++t) ln[t].qn = 0;
                if (!scanning) break;
            }
            if (roundsHere > longest) longest = roundsHere;
        }
    }
    for (int i = 0; i < kFcOut; ++i) out[i] = o[i];
    out[15] = longest;
}

// out[0] entries of the lists built last, out[1] those that carry no edge
__attribute__((visibility("default"))) void fc_edge_census(void* p, uint64_t* out)
{
    HcScene* s = static_cast<HcScene*>(p);
    uint64_t n = 0, none = 0;
    for (const DirCell& c : s->dmCells) {
        n += c.count;
        for (uint32_t k = 0; k < c.count; ++k) if (s->dmEntries[c.begin + k].edge == 0u) ++none;
    }
    out[0] = n; out[1] = none;
}

// A record made up by the caller (64 bytes, DirRecord) in texel (i, j) of an R-texel face: its entry by dm_local_entry, and for each of
// the 128 x 128 cells of the texel
//   passes[y * 128 + x]  the entry's edge term for a ray in that cell, dm_dot4(entry.edge, dm_ray_local(x, y).p) >= 0
//   real[y * 128 + x]    is the real-valued dilated triangle reached anywhere in the cell's closed square?  min over the three edges of
//                        the largest value of (p - P_k) . n_k + pad over the square (a linear function: at a corner), double, unit normals
//                        from double roots -- >= 0 means SOME edge function each is >= 0 there, the superset the one stored edge must keep
// `edgeMax` (3 x 128 x 128 doubles): that largest value per edge; *which: the edge the word stores (-1: none, or not identified) -- the
// byte test must pass wherever edgeMax[*which] >= 0.  Returns the entry's edge word.
__attribute__((visibility("default"))) uint32_t fc_edge_cells(const void* record, uint32_t R, uint32_t i, uint32_t j, uint8_t* passes, uint8_t* real, double* edgeMax,
                                                              int32_t* which)
{
    const DirRecord rec = *static_cast<const DirRecord*>(record);
    const DirEntry e = dm_local_entry(rec, R, i, j, 0u);
    const double area2 = ((double)rec.px[1] - rec.px[0]) * ((double)rec.py[2] - rec.py[0]) - ((double)rec.py[1] - rec.py[0]) * ((double)rec.px[2] - rec.px[0]);
    const double sgn = area2 > 0.0 ? 1.0 : -1.0;
    const double ou = 2.0 * i / R - 1.0, ov = 2.0 * j / R - 1.0, perCell = 1.0 / (64.0 * R);
    double nx[3], ny[3], c0[3];
    bool has[3];
    *which = -1;
    for (int k = 0; k < 3; ++k) {
        const double ex = (double)rec.px[(k + 1) % 3] - rec.px[k], ey = (double)rec.py[(k + 1) % 3] - rec.py[k];
        const double len = __builtin_sqrt(ex * ex + ey * ey);
        has[k] = (rec.hasTri & 1u) && len > 0.0;
        nx[k] = has[k] ? -ey / len * sgn : 0.0; ny[k] = has[k] ? ex / len * sgn : 0.0;
        c0[k] = (ou - rec.px[k]) * nx[k] + (ov - rec.py[k]) * ny[k] + rec.pad;
        // the stored edge is the one whose normal, scaled to 127 and rounded, gives the word's bytes a, b (no two edges of a triangle
        // point the same way; a rounding tie between this root and the builder's single-precision one is left as `not identified`)
        const double big = __builtin_fabs(nx[k]) > __builtin_fabs(ny[k]) ? __builtin_fabs(nx[k]) : __builtin_fabs(ny[k]);
        if (e.edge != 0u && has[k] && (int)__builtin_floor(nx[k] * 127.0 / big + 0.5) == (int)(int8_t)(e.edge & 0xffu) &&
            (int)__builtin_floor(ny[k] * 127.0 / big + 0.5) == (int)(int8_t)((e.edge >> 8) & 0xffu))
            *which = k;
    }
    for (uint32_t y = 0; y < kDmCells; ++y)
        for (uint32_t x = 0; x < kDmCells; ++x) {
            const size_t at = (size_t)y * kDmCells + x;
            passes[at] = dm_dot4(e.edge, dm_ray_local(x, y).p) >= 0 ? 1 : 0;
            double worst = 1e300;
            for (int k = 0; k < 3; ++k) {
                // largest value over [x, x + 1] x [y, y + 1]: each coordinate at the end its coefficient favours
                const double X = nx[k] > 0.0 ? x + 1.0 : (double)x, Y = ny[k] > 0.0 ? y + 1.0 : (double)y;
                const double v = has[k] ? c0[k] + (nx[k] * X + ny[k] * Y) * perCell : 1e300;
                if (edgeMax) edgeMax[((size_t)k * kDmCells + y) * kDmCells + x] = v;
                if (v < worst) worst = v;
            }
            real[at] = worst >= 0.0 ? 1 : 0;
        }
    return e.edge;
}

} // extern "C"
