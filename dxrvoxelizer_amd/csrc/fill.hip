// fill.hip -- the exterior flood fill of a whole N^3 grid (dxv_fill.h has the rule and the word routines), on the frame's stream:
//   k_fill_pack     grid (1 B per voxel) -> the free mask F and the seed of the reached mask R (1 bit each): the one read of the grid
//   k_fill_rows     a round's pass along x: one lane per row, carries from word to word
//   k_fill_columns  a round's passes along y and along z: one lane per 64-bit word column, adjacent lanes on adjacent words
//   k_fill_write    the masks -> the grid's bytes (0 / 1): the one write of the grid
// A batch is `rounds` rounds behind one another.  Whether a round changed a word is word `round` of the batch's control block; the
// kernels of a round return at once when the round before them left its word 0, so a batch costs what its live rounds cost, and the
// host reads the block where the frame is next synchronised (dxv_products.hip: settle_fill).  No workgroup waits for another, every
// loop is bounded by N; no LDS, no scratch memory.  The masks and the control block are laid out by fill_carve (dxv_fill.h).
#include "dxv_device.h"
#include "dxv_fill.h"

namespace dxv {

// one thread per byte of a mask row (W * 8 of them, the ones behind the row's end are 0)
__global__ __launch_bounds__(256) void k_fill_pack(const uint8_t* __restrict__ grid, uint32_t N, uint8_t* __restrict__ freeMask, uint8_t* __restrict__ reached)
{
    const uint32_t rowBytes = fill_row_words(N) * 8u;
    const size_t t = (size_t)blockIdx.x * 256u + threadIdx.x;
    if (t >= (size_t)N * N * rowBytes) return;
    const size_t row = t / rowBytes;
    const uint32_t j = (uint32_t)(t % rowBytes);
    uint32_t free8 = 0;
    if (8u * j < N) {
        const uint8_t* g = grid + row * N;
        free8 = (N & 7u) ? fill_free_byte(g, N, j) : fill_free_byte(*reinterpret_cast<const uint64_t*>(g + 8u * j));
    }
    freeMask[t] = (uint8_t)free8;
    reached[t] = (uint8_t)fill_seed_byte(free8, N, j, (uint32_t)(row % N), (uint32_t)(row / N));
}

__global__ __launch_bounds__(64) void k_fill_rows(const uint64_t* __restrict__ freeMask, uint64_t* __restrict__ reached, uint32_t N, uint32_t* __restrict__ ctl, uint32_t round)
{
    if (round && ctl[round - 1u] == 0u) return;
    const size_t row = (size_t)blockIdx.x * 64u + threadIdx.x;
    if (row >= (size_t)N * N) return;
    const uint32_t W = fill_row_words(N);
    if (fill_row(freeMask + row * W, reached + row * W, W)) ctl[round] = 1u;
}

// column i of `count` starts at word (i / inner) * outer + i % inner and steps by `stride` words
// (y pass: inner = W, outer = N W, stride = W -- i = iz * W + w; z pass: inner = count, stride = N W -- i = iy * W + w)
__global__ __launch_bounds__(64) void k_fill_columns(const uint64_t* __restrict__ freeMask, uint64_t* __restrict__ reached, uint32_t N, uint32_t count, uint32_t inner,
                                                     size_t outer, size_t stride, uint32_t* __restrict__ ctl, uint32_t round)
{
    if (round && ctl[round - 1u] == 0u) return;
    const uint32_t i = blockIdx.x * 64u + threadIdx.x;
    if (i >= count) return;
    const size_t base = (size_t)(i / inner) * outer + i % inner;
    FillColumn col{freeMask + base, reached + base, stride, N};
    if (col.run()) ctl[round] = 1u;
}

__global__ __launch_bounds__(256) void k_fill_write(const uint8_t* __restrict__ freeMask, const uint8_t* __restrict__ reached, uint32_t N, int what, uint8_t* __restrict__ grid)
{
    const uint32_t rowBytes = fill_row_words(N) * 8u;
    const size_t t = (size_t)blockIdx.x * 256u + threadIdx.x;
    if (t >= (size_t)N * N * rowBytes) return;
    const size_t row = t / rowBytes;
    const uint32_t j = (uint32_t)(t % rowBytes);
    if (8u * j >= N) return;
    const uint32_t bits = fill_result_byte(freeMask[t], reached[t], what);
    uint8_t* g = grid + row * N + 8u * j;
    if ((N & 7u) == 0u) *reinterpret_cast<uint64_t*>(g) = fill_spread_byte(bits);
    else
        for (uint32_t k = 0; k < 8u && 8u * j + k < N; ++k) g[k] = (uint8_t)((bits >> k) & 1u);
}

// One batch: (first: the pack,) `rounds` rounds, the write-back.  The control block is cleared in front of the rounds.
hipError_t launch_fill(uint8_t* grid, uint32_t N, int what, const FillScratch& l, uint32_t rounds, bool first, hipStream_t s)
{
    const uint32_t W = fill_row_words(N);
    const uint64_t* f = l.freeMask;
    uint64_t* r = l.reached;
    uint8_t* freeMask = reinterpret_cast<uint8_t*>(l.freeMask);
    uint8_t* reached = reinterpret_cast<uint8_t*>(l.reached);
    uint32_t* ctl = l.ctl;
    const size_t maskBytes = (size_t)N * N * W * 8u, rows = (size_t)N * N;
    const uint32_t byteBlocks = (uint32_t)((maskBytes + 255) / 256), columns = N * W;
    if (rounds < 1u) rounds = 1u;
    if (rounds > kFillMaxRounds) rounds = kFillMaxRounds;
    if (first) k_fill_pack<<<byteBlocks, 256, 0, s>>>(grid, N, freeMask, reached);
    const hipError_t e = hipMemsetAsync(ctl, 0, sizeof(uint32_t) * kFillMaxRounds, s);
    if (e != hipSuccess) return e;
    for (uint32_t k = 0; k < rounds; ++k) {
        k_fill_rows<<<(uint32_t)((rows + 63) / 64), 64, 0, s>>>(f, r, N, ctl, k);
        k_fill_columns<<<(columns + 63u) / 64u, 64, 0, s>>>(f, r, N, columns, W, (size_t)N * W, W, ctl, k);
        k_fill_columns<<<(columns + 63u) / 64u, 64, 0, s>>>(f, r, N, columns, columns, 0, (size_t)N * W, ctl, k);
    }
    k_fill_write<<<byteBlocks, 256, 0, s>>>(freeMask, reached, N, what, grid);
    return hipGetLastError();
}

} // namespace dxv
