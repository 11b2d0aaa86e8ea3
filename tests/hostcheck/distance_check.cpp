// The product's distance-field scans (dxrvoxelizer_amd/csrc/dxv_distance.h) compiled for the CPU: the same text the kernels of
// distance.hip run, driven here in the kernels' order -- rows along x, columns along y, columns along z.
#include "../../dxrvoxelizer_amd/csrc/dxv_distance.h"

#include <vector>

using namespace dxv;

extern "C" int dc_distance(const uint8_t* grid, uint32_t N, int format, int32_t* field)
{
    if (N < 2 || N > 2048 || (format != 0 && format != 1)) return 1;
    const size_t n2 = (size_t)N * N, n3 = n2 * N;
    std::vector<int16_t> rows(n3);
    std::vector<int32_t> squares(n3);
    const uint32_t W = (N + 63u) / 64u;
#pragma omp parallel for
    for (long long row = 0; row < (long long)n2; ++row) {
        uint64_t bits[32] = {};
        const uint8_t* g = grid + (size_t)row * N;
        for (uint32_t x = 0; x < N; ++x)
            if (g[x]) bits[x >> 6] |= 1ull << (x & 63u);
        (void)W;
        for (uint32_t x = 0; x < N; ++x) rows[(size_t)row * N + x] = (int16_t)dist_row_value(bits, N, x, g[x] != 0);
    }
#pragma omp parallel for
    for (long long i = 0; i < (long long)n2; ++i) {                     // i = iz * N + ix
        const size_t base = (size_t)(i / N) * n2 + (size_t)(i % N);
        DistColumn<int16_t, false> col{rows.data() + base, squares.data() + base, N, (int32_t)N};
        col.run();
    }
#pragma omp parallel for
    for (long long i = 0; i < (long long)n2; ++i) {                     // i = iy * N + ix
        if (format == 1) {
            DistColumn<int32_t, true> col{squares.data() + i, field + i, n2, (int32_t)N};
            col.run();
        } else {
            DistColumn<int32_t, false> col{squares.data() + i, field + i, n2, (int32_t)N};
            col.run();
        }
    }
    return 0;
}
