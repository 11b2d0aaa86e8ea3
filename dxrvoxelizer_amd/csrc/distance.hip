// distance.hip -- the exact signed distance field of a whole N^3 grid (dxv_distance.h has the rule and the scans): three kernels on
// the frame's stream.
//   k_dist_rows     grid (1 B) -> signed 16-bit x distances (2 B): one wave per row, the row packed by ballot, bit scans per voxel
//   k_dist_columns  along y: 16-bit -> signed 32-bit squares (2 B read, 4 B written + the stack's traffic in the written column)
//   k_dist_columns  along z: 32-bit -> the field (4 B read, 4 B written)
// A column scan is one lane per column, adjacent lanes on adjacent x: every lane of a wave is at the same u, so the loads of the input
// and the stores of the result are whole 256-byte (128-byte for the 16-bit input) wave accesses; only the stack's slots, a + q per
// lane, spread -- over neighbouring lines of the same x range.  No LDS in the column scans, no scratch memory.  The two intermediate fields are
// laid out by distance_carve (dxv_distance.h).
#include "dxv_device.h"
#include "dxv_distance.h"

namespace dxv {

constexpr uint32_t kDistRowWaves = 4;          // rows per workgroup of k_dist_rows

__global__ __launch_bounds__(64 * kDistRowWaves) void k_dist_rows(const uint8_t* __restrict__ grid, uint32_t N, int16_t* __restrict__ rows)
{
    __shared__ uint64_t bits[kDistRowWaves][32];                       // N <= 2048: 32 words per row
    const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63u;
    const size_t row = (size_t)blockIdx.x * kDistRowWaves + wave;       // (iz * N + iy); N is even: N^2 rows are whole workgroups
    const uint32_t W = (N + 63u) / 64u;
    const uint8_t* g = grid + row * N;
    for (uint32_t c = 0; c < W; ++c) {
        const uint32_t x = c * 64u + lane;
        const uint64_t b = __ballot(x < N && g[x] != 0);
        if (lane == 0) bits[wave][c] = b;
    }
    __syncthreads();
    for (uint32_t c = 0; c < W; ++c) {
        const uint32_t x = c * 64u + lane;
        if (x < N) rows[row * N + x] = (int16_t)dist_row_value(bits[wave], N, x, (bits[wave][c] >> lane) & 1ull);
    }
}

// columns of `count` lanes: column i starts at element (i / N) * outer + i % N and steps by `stride`
// (y pass: outer = N^2, stride = N -- i = iz * N + ix; z pass: outer = N, stride = N^2 -- i = iy * N + ix)
template <class TIn, bool kFloat>
__global__ __launch_bounds__(64) void k_dist_columns(const TIn* __restrict__ in, int32_t* __restrict__ out, uint32_t N, size_t outer, size_t stride)
{
    const uint32_t i = blockIdx.x * 64u + threadIdx.x;
    if (i >= N * N) return;
    const size_t base = (size_t)(i / N) * outer + i % N;
    DistColumn<TIn, kFloat> col{in + base, out + base, stride, (int32_t)N};
    col.run();
}

// scratch: distance_scratch_bytes(N) bytes (dxv_distance.h: distance_carve), which whoever embeds them has taken from its own carve
hipError_t launch_distance(const uint8_t* grid, uint32_t N, int format, void* field, uint8_t* scratch, hipStream_t s)
{
    Carve c(scratch, distance_scratch_bytes(N));
    DistScratch l;
    distance_carve(c, N, l);
    int16_t* rows = l.rows;
    int32_t* squares = l.squares;
    const size_t n2 = (size_t)N * N;
    const uint32_t columns = (uint32_t)((n2 + 63) / 64);
    k_dist_rows<<<(uint32_t)(n2 / kDistRowWaves), 64 * kDistRowWaves, 0, s>>>(grid, N, rows);
    k_dist_columns<int16_t, false><<<columns, 64, 0, s>>>(rows, squares, N, n2, N);
    if (format == 1) k_dist_columns<int32_t, true><<<columns, 64, 0, s>>>(squares, static_cast<int32_t*>(field), N, N, n2);
    else k_dist_columns<int32_t, false><<<columns, 64, 0, s>>>(squares, static_cast<int32_t*>(field), N, N, n2);
    return hipGetLastError();
}

} // namespace dxv
