// scan.hip -- the exclusive scan of C interleaved 32-bit counts per word (C = 1: octree, components; C = 2: isosurface's {vertices, quads}), in
// place, with 64-bit sums, in three kernels so that no workgroup waits for another:
//   k_scan_block_sums  per workgroup of 256 threads x 4 consecutive words: the C sums of its 1024 words, interleaved, one entry per block
//   k_scan_sums        ONE workgroup of 1024: the exclusive scan of the block sums in place -- a thread takes ceil(blocks / 1024) consecutive blocks,
//                      the range of a thread behind the last block is empty -- and the C totals through a pointer
//   k_scan_add         the scan inside every block again, on top of the block's entry: every word becomes what stands in front of it, its low
//                      32 bits (the callers refuse a total that passes their cap before anything reads them)
// launch_scan_words does all three; launch_scan_sums the middle one alone, for the callers that make the sums of their blocks themselves
// (thickness.hip, partition.hip) and place the totals behind them.  Every loop is bounded, nothing goes to scratch memory, the LDS is the waves'
// sums of dxv_scan.h.
#include "dxv_device.h"
#include "dxv_scan.h"

namespace dxv {

constexpr uint32_t kScanBlock = 256;                                    // threads of a workgroup of the two outer kernels ...
constexpr uint32_t kScanItems = 4;                                      // ... and the consecutive words each of them takes
static_assert(kScanWords == kScanBlock * kScanItems, "scan_blocks (dxv_scratch.h) counts the words of one such workgroup");
constexpr uint32_t kScanSumsBlock = 1024;                               // threads of the one workgroup that scans the block sums

// what C interleaved counts add up to, and C consecutive words (counts or sums) <-> that
template <uint32_t C> struct ScanSum;
template <> struct ScanSum<1> { using T = unsigned long long; };
template <> struct ScanSum<2> { using T = ScanPair; };
template <class W> __device__ __forceinline__ void scan_load(unsigned long long& t, const W* at) { t = at[0]; }
template <class W> __device__ __forceinline__ void scan_load(ScanPair& t, const W* at) { t.a = at[0]; t.b = at[1]; }
template <class W> __device__ __forceinline__ void scan_store(W* at, unsigned long long t) { at[0] = (W)t; }
template <class W> __device__ __forceinline__ void scan_store(W* at, ScanPair t) { at[0] = (W)t.a; at[1] = (W)t.b; }

template <uint32_t C> __global__ __launch_bounds__(kScanBlock) void k_scan_block_sums(const uint32_t* __restrict__ counts, size_t words, unsigned long long* __restrict__ sums)
{
    using T = typename ScanSum<C>::T;
    const size_t first = ((size_t)blockIdx.x * kScanBlock + threadIdx.x) * kScanItems;
    T mine{};
    for (uint32_t k = 0; k < kScanItems; ++k)
        if (first + k < words) {
            T c;
            scan_load(c, counts + C * (first + k));
            mine = mine + c;
        }
    T total;
    (void)block_scan_exclusive<T, kScanBlock / 64u>(mine, total);
    if (threadIdx.x == 0) scan_store(sums + C * (size_t)blockIdx.x, total);
}

// sums[C b ..] -> the sums of the blocks in front of block b; totals[0 .. C) = the sums of all blocks
template <uint32_t C> __global__ __launch_bounds__(kScanSumsBlock) void k_scan_sums(unsigned long long* __restrict__ sums, uint32_t blocks, unsigned long long* __restrict__ totals)
{
    using T = typename ScanSum<C>::T;
    const uint32_t chunk = (blocks + kScanSumsBlock - 1u) / kScanSumsBlock;
    const uint32_t first = threadIdx.x * chunk < blocks ? threadIdx.x * chunk : blocks, last = first + chunk < blocks ? first + chunk : blocks;
    T mine{};
    for (uint32_t b = first; b < last; ++b) {
        T v;
        scan_load(v, sums + C * (size_t)b);
        mine = mine + v;
    }
    T total;
    T run = block_scan_exclusive<T, kScanSumsBlock / 64u>(mine, total);
    for (uint32_t b = first; b < last; ++b) {
        T v;
        scan_load(v, sums + C * (size_t)b);
        scan_store(sums + C * (size_t)b, run);
        run = run + v;
    }
    if (threadIdx.x == 0) scan_store(totals, total);
}

template <uint32_t C> __global__ __launch_bounds__(kScanBlock) void k_scan_add(uint32_t* __restrict__ counts, size_t words, const unsigned long long* __restrict__ sums)
{
    using T = typename ScanSum<C>::T;
    const size_t first = ((size_t)blockIdx.x * kScanBlock + threadIdx.x) * kScanItems;
    uint32_t c[kScanItems][C];                                          // (the counts stay 32-bit; they are widened where they are added)
    T mine{}, v;
#pragma unroll
    for (uint32_t k = 0; k < kScanItems; ++k) {
#pragma unroll
        for (uint32_t j = 0; j < C; ++j) c[k][j] = first + k < words ? counts[C * (first + k) + j] : 0u;
        scan_load(v, c[k]);
        mine = mine + v;
    }
    T total, front;
    scan_load(front, sums + C * (size_t)blockIdx.x);
    T run = block_scan_exclusive<T, kScanBlock / 64u>(mine, total) + front;
#pragma unroll
    for (uint32_t k = 0; k < kScanItems; ++k) {
        if (first + k < words) scan_store(counts + C * (first + k), run);
        scan_load(v, c[k]);
        run = run + v;
    }
}

template <uint32_t C> static hipError_t scan_words(uint32_t* counts, size_t words, unsigned long long* sums, unsigned long long* totals, hipStream_t s)
{
    const uint32_t blocks = scan_blocks(words);
    k_scan_block_sums<C><<<blocks, kScanBlock, 0, s>>>(counts, words, sums);
    k_scan_sums<C><<<1, kScanSumsBlock, 0, s>>>(sums, blocks, totals);
    k_scan_add<C><<<blocks, kScanBlock, 0, s>>>(counts, words, sums);
    return hipGetLastError();
}

// counts: `words` words of C counts each -> what stands in front of every word; sums: C * scan_blocks(words) words of scratch; totals: C words
hipError_t launch_scan_words(uint32_t* counts, uint32_t C, size_t words, unsigned long long* sums, unsigned long long* totals, hipStream_t s)
{
    if (!counts || !sums || !totals || !words || (words + kScanWords - 1u) / kScanWords > 0x7fffffffull) return hipErrorInvalidValue;
    return C == 1u ? scan_words<1>(counts, words, sums, totals, s) : C == 2u ? scan_words<2>(counts, words, sums, totals, s) : hipErrorInvalidValue;
}

// sums: `blocks` entries of C sums each -> what stands in front of every entry; totals: C words (which may stand right behind the sums)
hipError_t launch_scan_sums(unsigned long long* sums, uint32_t C, uint32_t blocks, unsigned long long* totals, hipStream_t s)
{
    if (!sums || !totals || !blocks || (C != 1u && C != 2u)) return hipErrorInvalidValue;
    if (C == 1u) k_scan_sums<1><<<1, kScanSumsBlock, 0, s>>>(sums, blocks, totals);
    else k_scan_sums<2><<<1, kScanSumsBlock, 0, s>>>(sums, blocks, totals);
    return hipGetLastError();
}

} // namespace dxv
