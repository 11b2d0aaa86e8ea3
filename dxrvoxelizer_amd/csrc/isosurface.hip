// isosurface.hip -- a closed triangle mesh from a float32 field of a whole N^3 grid by naive Surface Nets (dxv_isosurface.h has the rule),
// as count -> scan -> emit, so that vertices and triangles stand in cell order whatever the scheduling:
//   k_iso_count      one wave per 64 consecutive cells of a cell row along x.  A lane loads the four samples at its own x -- whole-wave
//                    accesses of consecutive floats -- and takes the four at x - 1 from the lane below it (lane 0 loads its own): four
//                    loads per cell, not eight.  A ballot of "has a vertex" is the run's 64-bit word: one BIT per cell; the wave stores it
//                    with its popcount and the number of crossing edges its cells own.
//   scan.hip         the exclusive scan of the two counts per word (launch_scan_words, IsoCounts as two interleaved counts), which also leaves
//                    the two totals, 64-bit.
//   k_iso_emit       the count kernel's mapping again: a cell's vertex goes to the word's base + the popcount of the lower lanes' bits,
//                    a neighbour cell's number comes from that cell's word and base, the cell's up to three quads go to the word's quad
//                    base + the lane's rank among the wave's owned crossing edges.
// No kernel here uses scratch memory or LDS, every loop is bounded and no workgroup waits for another.  The scratch is laid out by iso_carve
// (dxv_isosurface.h).
#include "dxv_device.h"
#include "dxv_isosurface.h"

namespace dxv {

struct IsoCellSamples { float s[8]; uint32_t cx, cy, cz; bool valid; };

// the eight corner samples of this lane's cell in word `word`: the upper four (dx = 1) loaded, the lower four from the lane below
__device__ __forceinline__ IsoCellSamples iso_lane_cell(const IsoParams& p, size_t word, uint32_t lane)
{
    const uint32_t W = iso_row_words(p.N), C = p.N + 1u;
    const size_t row = word / W;
    IsoCellSamples c;
    c.cx = (uint32_t)(word % W) * 64u + lane;
    c.cy = (uint32_t)(row % C);
    c.cz = (uint32_t)(row / C);
    c.valid = c.cx <= p.N;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const int32_t j = (int32_t)c.cy - 1 + (e & 1), k = (int32_t)c.cz - 1 + (e >> 1);
        const float hi = iso_sample(p.field, p.N, (int32_t)c.cx, j, k, p.iso, p.P);
        float lo = __shfl_up(hi, 1);
        if (lane == 0) lo = iso_sample(p.field, p.N, (int32_t)c.cx - 1, j, k, p.iso, p.P);
        c.s[e << 1] = lo;
        c.s[(e << 1) | 1] = hi;
    }
    return c;
}

__global__ __launch_bounds__(256) void k_iso_count(IsoParams p, size_t words)
{
    const size_t word = (size_t)blockIdx.x * 4u + (threadIdx.x >> 6);
    if (word >= words) return;                                          // (the whole wave)
    const uint32_t lane = threadIdx.x & 63u;
    const IsoCellSamples c = iso_lane_cell(p, word, lane);
    const bool active = c.valid && iso_active(c.s);
    const uint32_t owned = c.valid ? iso_owned(c.s) : 0u;
    const uint64_t mask = __ballot(active);
    const uint32_t quads = iso_popc(__ballot(owned & 1u)) + iso_popc(__ballot(owned & 2u)) + iso_popc(__ballot(owned & 4u));
    if (lane == 0) {
        p.masks[word] = mask;
        p.bases[word] = IsoCounts{iso_popc(mask), quads};
    }
}

__global__ __launch_bounds__(256) void k_iso_emit(IsoParams p, size_t words)
{
    const size_t word = (size_t)blockIdx.x * 4u + (threadIdx.x >> 6);
    if (word >= words) return;
    const uint32_t lane = threadIdx.x & 63u;
    const IsoCellSamples c = iso_lane_cell(p, word, lane);
    const bool active = c.valid && iso_active(c.s);
    const uint32_t owned = c.valid ? iso_owned(c.s) : 0u;
    const uint64_t mask = __ballot(active), lower = (1ull << lane) - 1ull;
    const uint64_t bx = __ballot(owned & 1u), by = __ballot(owned & 2u), bz = __ballot(owned & 4u);
    if (!active) return;                                                // (a cell that owns a crossing edge is active)
    const IsoCounts base = p.bases[word];
    const bool object = p.object != 0;
    IsoVertex v = iso_vertex(c.s, c.cx, c.cy, c.cz);
    if (object) iso_to_object(v, p.N, p.bound);
    p.vb[base.vertices + iso_popc(mask & lower)] = v;
    if (!owned) return;
    const uint32_t cell[3] = {c.cx, c.cy, c.cz};
    uint32_t quad = base.quads + iso_popc(bx & lower) + iso_popc(by & lower) + iso_popc(bz & lower);
    const bool firstInside = iso_inside(c.s[0]);
#pragma unroll
    for (int axis = 0; axis < 3; ++axis) {
        if (!(owned & (1u << axis))) continue;
        if (!cell[(axis + 1) % 3] || !cell[(axis + 2) % 3]) continue;   // (never: both ends of such an edge lie in the padding, and it does not cross)
        uint32_t out[6];
        iso_quad(out, p.masks, p.bases, p.N, c.cx, c.cy, c.cz, axis, firstInside, object);
        uint32_t* dst = p.ib + 6 * (size_t)quad;
#pragma unroll
        for (int k = 0; k < 6; ++k) dst[k] = out[k];
        ++quad;
    }
}

// count + scan: p.masks and p.bases (what stands in front of every word) and p.totals = {vertices, quads} of the whole mesh
hipError_t launch_iso_count(const IsoParams& p, hipStream_t s)
{
    const size_t words = iso_words(p.N), waveBlocks = (words + 3u) / 4u;
    if (!p.N || p.N > 2048u || waveBlocks > 0x7fffffffull) return hipErrorInvalidValue;
    static_assert(sizeof(IsoCounts) == 8, "the scan takes a word's {vertices, quads} as two interleaved 32-bit counts");
    k_iso_count<<<(uint32_t)waveBlocks, 256, 0, s>>>(p, words);
    return launch_scan_words(reinterpret_cast<uint32_t*>(p.bases), 2, words, p.sums, p.totals, s);
}

// emit: p.vb (totals[0] vertices) and p.ib (6 x totals[1] index words) from what launch_iso_count left
hipError_t launch_iso_emit(const IsoParams& p, hipStream_t s)
{
    const size_t words = iso_words(p.N), waveBlocks = (words + 3u) / 4u;
    if (!p.N || p.N > 2048u || waveBlocks > 0x7fffffffull || !p.vb) return hipErrorInvalidValue;
    k_iso_emit<<<(uint32_t)waveBlocks, 256, 0, s>>>(p, words);
    return hipGetLastError();
}

} // namespace dxv
