// The product's thickness routines (csrc/dxv_thickness.h) compiled for the CPU: the same chain as csrc/thickness.hip -- the field of the grid, E
// and its field, Top, Top's field, the select, the paint, the histogram -- with loops where the device has grids of threads and a plain maximum
// where it has an atomic one.  The fields are the product's own scans (csrc/dxv_distance.h) in the kernels' order.  tests/thickness_host.py
// loads this; tests/test_thickness_rule.py compares it with the numpy restatement.
#include <stdint.h>
#include <string.h>
#include <vector>
#include "../../dxrvoxelizer_amd/csrc/dxv_distance.h"
#include "../../dxrvoxelizer_amd/csrc/dxv_thickness.h"

using namespace dxv;

static void field_of(const uint8_t* grid, uint32_t N, int32_t* field)
{
    const size_t n2 = (size_t)N * N, n3 = n2 * N;
    std::vector<int16_t> rows(n3);
    std::vector<int32_t> squares(n3);
    for (size_t row = 0; row < n2; ++row) {
        uint64_t bits[32] = {};
        const uint8_t* g = grid + row * N;
        for (uint32_t x = 0; x < N; ++x)
            if (g[x]) bits[x >> 6] |= 1ull << (x & 63u);
        for (uint32_t x = 0; x < N; ++x) rows[row * N + x] = (int16_t)dist_row_value(bits, N, x, g[x] != 0);
    }
    for (size_t i = 0; i < n2; ++i) {                                   // i = iz * N + ix
        const size_t base = (i / N) * n2 + i % N;
        DistColumn<int16_t, false> col{rows.data() + base, squares.data() + base, N, (int32_t)N};
        col.run();
    }
    for (size_t i = 0; i < n2; ++i) {                                   // i = iy * N + ix
        DistColumn<int32_t, false> col{squares.data() + i, field + i, n2, (int32_t)N};
        col.run();
    }
}

extern "C" {

// grid: N^3 bytes; W: N^3 uint32, written; hist: cap + 1 uint64, written; counters: {centres painted, work items}, written
int tc_thickness(const uint8_t* grid, uint32_t N, int of, uint32_t cap, uint32_t cull, uint32_t* W, uint64_t* hist, uint64_t* counters)
{
    if (N < 2u || N > kThickMaxN || (N & 1u) || (of != THICK_SOLID && of != THICK_EMPTY) || cap < kThickMinCapSq || cap > kThickMaxCapSq || cull > 3u) return 1;
    const size_t n3 = (size_t)N * N * N;
    std::vector<int32_t> F(n3), G(n3);
    std::vector<uint8_t> B(n3);
    field_of(grid, N, F.data());
    for (size_t v = 0; v < n3; ++v) B[v] = thick_radius(F[v], of, cap) == cap;
    field_of(B.data(), N, G.data());
    for (size_t v = 0; v < n3; ++v) {
        B[v] = (uint8_t)thick_top(B[v], G[v], cap);
        W[v] = B[v] ? cap : thick_radius(F[v], of, cap);
    }
    if (cull & THICK_CULL_TOP) field_of(B.data(), N, G.data());
    counters[0] = counters[1] = 0;
    for (uint32_t z = 0; z < N; ++z)
        for (uint32_t y = 0; y < N; ++y)
            for (uint32_t x = 0; x < N; ++x) {
                const uint32_t items = thick_items(F.data(), G.data(), N, x, y, z, of, cap, cull);
                if (!items) continue;
                ++counters[0];
                counters[1] += items;
                const uint32_t R = thick_radius(F[((size_t)z * N + y) * N + x], of, cap), first = thick_disc_first(z, thick_reach(R));
                for (uint32_t k = 0; k < items; ++k)
                    thick_paint_disc(N, x, y, z, R, first + k, 0u, 1u, [&](size_t at, uint32_t r) { if (W[at] < r) W[at] = r; });
            }
    memset(hist, 0, ((size_t)cap + 1u) * sizeof(uint64_t));
    for (size_t v = 0; v < n3; ++v) {
        if (W[v] > cap) return 2;
        ++hist[W[v]];
    }
    return 0;
}

uint32_t tc_max_n(void) { return kThickMaxN; }
uint32_t tc_isqrt(uint32_t v) { return thick_isqrt(v); }

}
