// isosurface.hip -- a closed triangle mesh from a float32 field of a whole N^3 grid by naive Surface Nets (dxv_isosurface.h has the rule),
// as count -> scan -> emit, so that vertices and triangles stand in cell order whatever the scheduling:
//   k_iso_count      one wave per 64 consecutive cells of a cell row along x.  A lane loads the four samples at its own x -- whole-wave
//                    accesses of consecutive floats -- and takes the four at x - 1 from the lane below it (lane 0 loads its own): four
//                    loads per cell, not eight.  A ballot of "has a vertex" is the run's 64-bit word: one BIT per cell; the wave stores it
//                    with its popcount and the number of crossing edges its cells own.
//   k_iso_block_sums, k_iso_scan_sums, k_iso_add
//                    the exclusive scan of the two counts per word: sums of blocks of 1024 words, the scan of the sums by one workgroup
//                    (which also leaves the two totals, 64-bit), the scan inside every block on top of its sum.  Every loop is bounded
//                    and no workgroup waits for another.
//   k_iso_emit       the count kernel's mapping again: a cell's vertex goes to the word's base + the popcount of the lower lanes' bits,
//                    a neighbour cell's number comes from that cell's word and base, the cell's up to three quads go to the word's quad
//                    base + the lane's rank among the wave's owned crossing edges.
// No kernel uses scratch memory; the scan's kernels use 256 bytes of LDS per workgroup (the waves' sums), the other two none.
#include "dxv_device.h"
#include "dxv_isosurface.h"

namespace dxv {

constexpr uint32_t kIsoScanBlock = 256;                                 // threads of a scan workgroup ...
constexpr uint32_t kIsoScanItems = 4;                                   // ... and the consecutive words each of them takes
constexpr uint32_t kIsoScanWords = kIsoScanBlock * kIsoScanItems;
constexpr uint32_t kIsoSumsBlock = 1024;                                // threads of the one workgroup that scans the block sums

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

struct IsoPair { unsigned long long v, q; };

// exclusive scan of one pair per thread over the workgroup (blockDim.x a multiple of 64, at most 1024); total: the workgroup's sum
__device__ __forceinline__ IsoPair iso_block_scan(IsoPair mine, IsoPair& total)
{
    __shared__ unsigned long long waveSums[2][16];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6, waves = blockDim.x >> 6;
    IsoPair inc = mine;
#pragma unroll
    for (uint32_t d = 1; d < 64u; d <<= 1) {
        const unsigned long long v = __shfl_up(inc.v, d), q = __shfl_up(inc.q, d);
        if (lane >= d) { inc.v += v; inc.q += q; }
    }
    if (lane == 63u) { waveSums[0][wave] = inc.v; waveSums[1][wave] = inc.q; }
    __syncthreads();
    IsoPair before{0, 0};
    total = IsoPair{0, 0};
    for (uint32_t k = 0; k < waves; ++k) {
        if (k < wave) { before.v += waveSums[0][k]; before.q += waveSums[1][k]; }
        total.v += waveSums[0][k]; total.q += waveSums[1][k];
    }
    __syncthreads();                                                    // (the sums may be written again by the caller's next scan)
    return IsoPair{before.v + inc.v - mine.v, before.q + inc.q - mine.q};
}

__global__ __launch_bounds__(kIsoScanBlock) void k_iso_block_sums(const IsoCounts* __restrict__ counts, size_t words, unsigned long long* __restrict__ sums)
{
    const size_t first = ((size_t)blockIdx.x * kIsoScanBlock + threadIdx.x) * kIsoScanItems;
    IsoPair mine{0, 0};
    for (uint32_t k = 0; k < kIsoScanItems; ++k)
        if (first + k < words) { mine.v += counts[first + k].vertices; mine.q += counts[first + k].quads; }
    IsoPair total;
    (void)iso_block_scan(mine, total);
    if (threadIdx.x == 0) { sums[2 * (size_t)blockIdx.x] = total.v; sums[2 * (size_t)blockIdx.x + 1] = total.q; }
}

// sums[2 b], sums[2 b + 1] -> the sums of the blocks in front of block b; totals[0], totals[1] = the sums of all blocks
__global__ __launch_bounds__(kIsoSumsBlock) void k_iso_scan_sums(unsigned long long* __restrict__ sums, uint32_t blocks, unsigned long long* __restrict__ totals)
{
    const uint32_t chunk = (blocks + kIsoSumsBlock - 1u) / kIsoSumsBlock;
    const uint32_t first = threadIdx.x * chunk, last = first + chunk < blocks ? first + chunk : blocks;
    IsoPair mine{0, 0};
    for (uint32_t b = first; b < last; ++b) { mine.v += sums[2 * (size_t)b]; mine.q += sums[2 * (size_t)b + 1]; }
    IsoPair total;
    IsoPair run = iso_block_scan(mine, total);
    for (uint32_t b = first; b < last; ++b) {
        const unsigned long long v = sums[2 * (size_t)b], q = sums[2 * (size_t)b + 1];
        sums[2 * (size_t)b] = run.v; sums[2 * (size_t)b + 1] = run.q;
        run.v += v; run.q += q;
    }
    if (threadIdx.x == 0) { totals[0] = total.v; totals[1] = total.q; }
}

// counts -> what stands in front of every word, in place (32-bit: a mesh whose totals pass the cap is refused before anything reads them)
__global__ __launch_bounds__(kIsoScanBlock) void k_iso_add(IsoCounts* __restrict__ counts, size_t words, const unsigned long long* __restrict__ sums)
{
    const size_t first = ((size_t)blockIdx.x * kIsoScanBlock + threadIdx.x) * kIsoScanItems;
    IsoCounts c[kIsoScanItems];
    IsoPair mine{0, 0};
#pragma unroll
    for (uint32_t k = 0; k < kIsoScanItems; ++k) {
        c[k] = first + k < words ? counts[first + k] : IsoCounts{0, 0};
        mine.v += c[k].vertices; mine.q += c[k].quads;
    }
    IsoPair total;
    IsoPair run = iso_block_scan(mine, total);
    run.v += sums[2 * (size_t)blockIdx.x]; run.q += sums[2 * (size_t)blockIdx.x + 1];
#pragma unroll
    for (uint32_t k = 0; k < kIsoScanItems; ++k) {
        if (first + k < words) counts[first + k] = IsoCounts{(uint32_t)run.v, (uint32_t)run.q};
        run.v += c[k].vertices; run.q += c[k].quads;
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

static uint32_t iso_scan_blocks(uint32_t N) { return (uint32_t)((iso_words(N) + kIsoScanWords - 1u) / kIsoScanWords); }

// scratch of one extraction: the words' masks, their counts / bases, the scan's block sums, the two totals
size_t iso_scratch_bytes(uint32_t N)
{
    const size_t words = iso_words(N);
    return words * sizeof(uint64_t) + words * sizeof(IsoCounts) + 2 * (size_t)iso_scan_blocks(N) * sizeof(unsigned long long) + 2 * sizeof(unsigned long long);
}
void iso_scratch_layout(uint8_t* scratch, uint32_t N, IsoParams& p)
{
    const size_t words = iso_words(N);
    p.masks = reinterpret_cast<uint64_t*>(scratch);
    p.bases = reinterpret_cast<IsoCounts*>(scratch + words * sizeof(uint64_t));
    p.sums = reinterpret_cast<unsigned long long*>(scratch + words * (sizeof(uint64_t) + sizeof(IsoCounts)));
    p.totals = p.sums + 2 * (size_t)iso_scan_blocks(N);
}

// count + scan: p.masks and p.bases (what stands in front of every word) and p.totals = {vertices, quads} of the whole mesh
hipError_t launch_iso_count(const IsoParams& p, hipStream_t s)
{
    const size_t words = iso_words(p.N), waveBlocks = (words + 3u) / 4u;
    if (!p.N || p.N > 2048u || waveBlocks > 0x7fffffffull) return hipErrorInvalidValue;
    const uint32_t blocks = iso_scan_blocks(p.N);
    k_iso_count<<<(uint32_t)waveBlocks, 256, 0, s>>>(p, words);
    k_iso_block_sums<<<blocks, kIsoScanBlock, 0, s>>>(p.bases, words, p.sums);
    k_iso_scan_sums<<<1, kIsoSumsBlock, 0, s>>>(p.sums, blocks, p.totals);
    k_iso_add<<<blocks, kIsoScanBlock, 0, s>>>(p.bases, words, p.sums);
    return hipGetLastError();
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
