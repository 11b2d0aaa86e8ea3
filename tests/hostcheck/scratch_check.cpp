// The operators' scratch descriptions (the X_carve functions of dxrvoxelizer_amd/csrc/dxv_*.h over dxv_scratch.h's Carve) compiled for the CPU:
// one row = one operator at one set of arguments, carved over a base the caller names (0: none, the sizing run) -- the bytes used, whether they
// fit the capacity, and every pointer the carve stored as an offset from the base (-1: null).  tests/scratch_host.py reads the rows as text;
// tests/cpp/scratch_sanitize_main.cpp carves into allocations of exactly the bytes asked for and writes to both ends of every block.
#include "../../dxrvoxelizer_amd/csrc/dxv_access.h"
#include "../../dxrvoxelizer_amd/csrc/dxv_components.h"
#include "../../dxrvoxelizer_amd/csrc/dxv_isosurface.h"
#include "../../dxrvoxelizer_amd/csrc/dxv_morph.h"
#include "../../dxrvoxelizer_amd/csrc/dxv_octree.h"
#include "../../dxrvoxelizer_amd/csrc/dxv_partition.h"
#include "../../dxrvoxelizer_amd/csrc/dxv_skeleton.h"
#include "../../dxrvoxelizer_amd/csrc/dxv_thin.h"

#include <stdio.h>
#include <string.h>
#include <string>
#include <utility>
#include <vector>

using namespace dxv;

struct ScratchRow {
    size_t used = 0;
    bool fits = false;
    std::vector<std::pair<const char*, const void*>> at;
};

static void thick_pointers(ScratchRow& r, const ThickParams& p)
{
    r.at.insert(r.at.end(), {{"F", p.F}, {"G", p.G}, {"B", p.B}, {"sums", p.sums}, {"passes", p.passes}, {"centres", p.centres}, {"firstItem", p.firstItem}, {"counters", p.counters}});
}

// op: the operator's name in tests/golden/operator_scratch.json; a: its arguments there.  false: no such operator
bool scratch_row(const char* name, const unsigned long long* a, uint8_t* base, size_t capacity, ScratchRow& r)
{
    const std::string op = name;
    const uint32_t N = (uint32_t)a[0];
    Carve c(base, capacity);
    if (op == "comp") { CompParams p{}; comp_carve(c, N, p); r.at = {{"mask", p.mask}, {"rootMask", p.rootMask}, {"bases", p.bases}, {"sums", p.sums}, {"total", p.total}}; }
    else if (op == "comp_select") { CompSelectWork w{}; comp_select_carve(c, (uint32_t)a[0], w); r.at = {{"counters", w.counters}, {"keep", w.keep}}; }
    else if (op == "skel") {
        SkelParams p{};
        skel_carve(c, N, p);
        r.at = {{"member", p.member}, {"node", p.node}, {"curve", p.curve}, {"ends", p.ends}, {"nodeRoots", p.nodeRoots}, {"curveRoots", p.curveRoots}, {"counts", p.counts}, {"sums", p.sums},
                {"totals", p.totals}};
    }
    else if (op == "skel_prune") { SkelPruneWork w{}; skel_prune_carve(c, (uint32_t)a[0], (uint32_t)a[1], w); r.at = {{"counters", w.counters}, {"goB", w.goB}, {"goN", w.goN}}; }
    else if (op == "oct") { OctParams p{}; oct_carve(c, N, p); r.at = {{"cells", p.cells}, {"masks", p.masks}, {"bases", p.bases}, {"sums", p.sums}, {"levelFirst", p.levelFirst}}; }
    else if (op == "iso") { IsoParams p{}; iso_carve(c, N, p); r.at = {{"masks", p.masks}, {"bases", p.bases}, {"sums", p.sums}, {"totals", p.totals}}; }
    else if (op == "thick") { ThickParams p{}; thickness_carve(c, N, p); thick_pointers(r, p); }
    else if (op == "part") {
        PartParams p{};
        partition_carve(c, N, p);
        r.at = {{"F", p.F}, {"parent", p.parent}, {"number", p.number}, {"rootOf", p.rootOf}, {"keys", p.keys}, {"mip4", p.mip4}, {"mip16", p.mip16}, {"sums", p.sums},
                {"counters", p.counters}, {"passes", p.passes}, {"totals", p.totals}};
    }
    else if (op == "part_work") {
        PartParams p{};
        partition_work_carve(c, (uint32_t)a[0], a[1], p);
        r.at = {{"stats", p.stats}, {"sortA", p.sortA}, {"sortB", p.sortB}, {"hist", p.hist}, {"headSums", p.headSums}, {"pairCount", p.pairCount}, {"pairTotal", p.pairTotal}};
    }
    else if (op == "access") {
        AccScratch l{};
        access_carve(c, N, a[1] != 0, l);
        r.at = {{"ctl", l.ctl}, {"seedsUsed", l.seedsUsed}, {"flags0", l.flags[0]}, {"flags1", l.flags[1]}, {"queue", l.queue}};
        thick_pointers(r, l.thick);
    }
    else if (op == "geo") { GeoScratch l{}; geodesic_carve(c, N, l); r.at = {{"ctl", l.ctl}, {"flags0", l.flags[0]}, {"flags1", l.flags[1]}, {"queue", l.queue}}; }
    else if (op == "fill") { FillScratch l{}; fill_carve(c, N, l); r.at = {{"free", l.freeMask}, {"reached", l.reached}, {"ctl", l.ctl}}; }
    else if (op == "thin") { ThinScratch l{}; thin_carve(c, N, l); r.at = {{"ctl", l.ctl}, {"S", l.S}, {"was", l.was}, {"B", l.B}, {"loose", l.loose}}; }
    else if (op == "dist") { DistScratch l{}; distance_carve(c, N, l); r.at = {{"rows", l.rows}, {"squares", l.squares}}; }
    else if (op == "morph") {
        MorphScratch l{};
        morph_carve(c, N, (int)a[1], (uint32_t)a[2], (int)a[3], l);
        r.at = {{"counters", l.counters}};
        if ((int)a[3] == MORPH_FORM_FIELD) r.at.insert(r.at.end(), {{"field", l.field}, {"passes", l.passes}});
        else r.at.insert(r.at.end(), {{"packed", l.packed}, {"half0", l.half[0]}, {"half1", l.half[1]}, {"loose", l.loose}, {"planes", l.planes}});
    }
    else return false;
    r.used = c.used();
    r.fits = c.fits();
    return true;
}

// "used fits name=offset ..." into out; returns its length, -1: no such operator or no room
extern "C" int sc_row(const char* op, const unsigned long long* args, unsigned long long base, unsigned long long capacity, char* out, int room)
{
    ScratchRow r;
    uint8_t* b = reinterpret_cast<uint8_t*>((uintptr_t)base);
    if (!scratch_row(op, args, b, (size_t)capacity, r)) return -1;
    int n = snprintf(out, (size_t)room, "%zu %d", r.used, r.fits ? 1 : 0);
    for (const auto& p : r.at) {
        if (n < 0 || n >= room) return -1;
        const long long off = p.second ? (long long)(static_cast<const uint8_t*>(p.second) - b) : -1ll;
        n += snprintf(out + n, (size_t)(room - n), " %s=%lld", p.first, off);
    }
    return n < room ? n : -1;
}
extern "C" unsigned long long sc_oct_levels(uint32_t N) { return oct_levels(N); }
