// The product's partition routines (csrc/dxv_partition.h) compiled for the CPU: the same chain as csrc/partition.hip -- the field of the grid, the
// keys and their two mip levels, the pruned parent search, the chain walk, the numbering, the labels, the regions' stats, the throats -- with
// loops where the device has grids of threads, plain updates where it has atomics and std::sort where it has the radix sort.  The field is the
// product's own scans (csrc/dxv_distance.h) in the kernels' order.  The centres of the search are taken forwards, backwards or shuffled: the
// argmax does not depend on it.  tests/partition_host.py loads this; tests/test_partition_rule.py compares it with the numpy restatement.
#include <stdint.h>
#include <string.h>
#include <algorithm>
#include <numeric>
#include <vector>
#include "../../dxrvoxelizer_amd/csrc/dxv_distance.h"
#include "../../dxrvoxelizer_amd/csrc/dxv_partition.h"

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

static std::vector<uint32_t> g_labels;
static std::vector<PartRegion> g_table;
static std::vector<PartThroat> g_throats;

extern "C" {

// grid: N^3 bytes; order: 0 = the centres forwards, 1 = backwards, 2 = shuffled (a fixed permutation).  counts: {K, T, interface faces, mip cells
// tested, voxels tested}, written.  The labels, the table and the throats stay here until the next call: pc_fetch copies them out.
int pc_partition(const uint8_t* grid, uint32_t N, int of, uint32_t cap, uint32_t prune, int order, int wantThroats, uint64_t* counts)
{
    if (N < 2u || N > kThickMaxN || (N & 1u) || (of != PART_SOLID && of != PART_EMPTY) || cap < kPartMinCapSq || cap > kPartMaxCapSq || prune > 3u) return 1;
    const uint32_t n3 = N * N * N, n4 = part_cells(N, 4u), n16 = part_cells(N, 16u);
    std::vector<int32_t> F(n3);
    field_of(grid, N, F.data());
    std::vector<uint64_t> keys(n3), mip4((size_t)n4 * n4 * n4), mip16((size_t)n16 * n16 * n16);
    for (uint32_t v = 0; v < n3; ++v) keys[v] = part_key(thick_radius(F[v], of, cap), v);
    for (uint32_t bz = 0; bz < n4; ++bz)
        for (uint32_t by = 0; by < n4; ++by)
            for (uint32_t bx = 0; bx < n4; ++bx) mip4[((size_t)bz * n4 + by) * n4 + bx] = part_mip4_of(keys.data(), N, bx, by, bz);
    for (uint32_t cz = 0; cz < n16; ++cz)
        for (uint32_t cy = 0; cy < n16; ++cy)
            for (uint32_t cx = 0; cx < n16; ++cx) mip16[((size_t)cz * n16 + cy) * n16 + cx] = part_mip16_of(mip4.data(), n4, cx, cy, cz);

    std::vector<uint32_t> parent(n3, kPartNone), rootOf(n3, kPartNone), number(n3, 0u);
    uint64_t cells = 0, voxels = 0;
    uint32_t stride = 1;                                                // shuffled: v -> (v * stride + 7) mod n3, stride odd and coprime to n3
    if (order == 2) { stride = 2654435761u % n3 | 1u; while (std::gcd(stride, n3) != 1u) stride += 2u; }
    for (uint32_t t = 0; t < n3; ++t) {
        const uint32_t v = order == 0 ? t : order == 1 ? n3 - 1u - t : (uint32_t)(((uint64_t)t * stride + 7u) % n3);
        const uint32_t R = part_key_radius(keys[v]);
        if (!R) continue;
        const uint32_t row = v / N;
        PartSearch<true> s{keys.data(), mip4.data(), mip16.data(), N, prune, v - row * N, row % N, row / N, R, 0, 0, 0};
        parent[v] = part_key_index(s.run());
        cells += s.cells;
        voxels += s.voxels;
    }
    for (uint32_t v = 0; v < n3; ++v)
        if (keys[v]) rootOf[v] = part_root(parent.data(), v, n3);
    uint32_t K = 0;
    for (uint32_t v = 0; v < n3; ++v)
        if (rootOf[v] == v) number[v] = ++K;
    g_labels.assign(n3, 0u);
    for (uint32_t v = 0; v < n3; ++v)
        if (rootOf[v] != kPartNone) g_labels[v] = number[rootOf[v]];

    std::vector<PartStats> stats(K, part_stats_none());
    for (uint32_t z = 0, v = 0; z < N; ++z)
        for (uint32_t y = 0; y < N; ++y)
            for (uint32_t x = 0; x < N; ++x, ++v) {
                if (!g_labels[v]) continue;
                PartStats& s = stats[g_labels[v] - 1u];
                const uint32_t c[3] = {x, y, z};
                ++s.voxels;
                for (int k = 0; k < 3; ++k) { s.lo[k] = std::min(s.lo[k], c[k]); s.hi[k] = std::max(s.hi[k], c[k]); }
                s.flags |= part_border(x, y, z, N);
            }
    g_table.assign(K, PartRegion{});
    for (uint32_t v = 0; v < n3; ++v)
        if (rootOf[v] == v) g_table[number[v] - 1u] = part_region(v, part_key_radius(keys[v]), stats[number[v] - 1u]);

    g_throats.clear();
    uint64_t faces = 0;
    if (wantThroats) {
        const uint32_t shift = part_label_bits(K);
        std::vector<uint64_t> pairs;
        for (uint32_t z = 0, v = 0; z < N; ++z)
            for (uint32_t y = 0; y < N; ++y)
                for (uint32_t x = 0; x < N; ++x, ++v) {
                    uint32_t other[3];
                    const uint32_t bits = part_faces(g_labels.data(), 0u, N, x, y, z, other);
                    for (uint32_t k = 0; k < 3u; ++k)
                        if (bits >> k & 1u) pairs.push_back(part_pair(g_labels[v], other[k], shift));
                }
        faces = pairs.size();
        std::sort(pairs.begin(), pairs.end());
        pairs.erase(std::unique(pairs.begin(), pairs.end()), pairs.end());
        const uint32_t T = (uint32_t)pairs.size();
        std::vector<uint32_t> count(T, 0u);
        std::vector<uint64_t> neck(T, 0ull);
        const uint32_t step[3] = {1u, N, N * N};
        for (uint32_t z = 0, v = 0; z < N; ++z)
            for (uint32_t y = 0; y < N; ++y)
                for (uint32_t x = 0; x < N; ++x, ++v) {
                    uint32_t other[3];
                    const uint32_t bits = part_faces(g_labels.data(), 0u, N, x, y, z, other);
                    for (uint32_t k = 0; k < 3u; ++k) {
                        if (!(bits >> k & 1u)) continue;
                        const uint32_t t = part_find_pair(pairs.data(), T, part_pair(g_labels[v], other[k], shift));
                        if (t >= T) return 3;
                        ++count[t];
                        neck[t] = std::max(neck[t], part_neck_word(std::min(part_key_radius(keys[v]), part_key_radius(keys[v + step[k]])), v));
                    }
                }
        for (uint32_t t = 0; t < T; ++t) {
            g_throats.push_back(part_throat(pairs[t], shift, count[t], neck[t]));
            ++g_table[g_throats[t].a - 1u].throats;
            ++g_table[g_throats[t].b - 1u].throats;
        }
    }
    counts[0] = K; counts[1] = g_throats.size(); counts[2] = faces; counts[3] = cells; counts[4] = voxels;
    return 0;
}

// labels: N^3 uint32; table: 32 K bytes; throats: 20 T bytes
void pc_fetch(uint32_t* labels, void* table, void* throats)
{
    memcpy(labels, g_labels.data(), g_labels.size() * sizeof(uint32_t));
    if (!g_table.empty()) memcpy(table, g_table.data(), g_table.size() * sizeof(PartRegion));
    if (!g_throats.empty()) memcpy(throats, g_throats.data(), g_throats.size() * sizeof(PartThroat));
}

}
